"""The stand-alone check programs of the plain-C++ plan headers, without a GPU: every
muscato_amd/csrc/host/*_check.cpp is listed in build.CHECKS with the headers it includes, is built by muscato_amd/build.py
next to the tools and run, and is built again with AddressSanitizer and UBSan and run.  Each reports how many checks it
evaluated: never fewer than build.CHECKS records, and the same number both ways."""
import functools
import glob
import os
import re
import subprocess

import pytest

from muscato_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muscato_amd", "csrc")
NAMES = sorted(mbuild.CHECKS)


def run(exe, name):
    """-> (the N of the one stdout line "NAME: N checks passed", stderr); the program has left with status 0."""
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout
    m = re.fullmatch(re.escape(name) + r": (\d+) checks passed( \(.+\))?", lines[0])
    assert m, r.stdout
    return int(m.group(1)), r.stderr


@functools.lru_cache(maxsize=None)
def plain_checks(name):
    return run(mbuild.build_checks()[name], name)[0]


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """Programs of their own with their own main: compiled with -fsanitize=address,undefined, the runtimes linked in."""
    return mbuild.build_checks(force=True, sanitize=True, out_dir=str(tmp_path_factory.mktemp("checks_san")))


def test_every_check_program_is_listed():
    on_disk = {os.path.basename(p)[:-len(".cpp")] for p in glob.glob(os.path.join(CSRC, "host", "*_check.cpp"))}
    assert on_disk == set(mbuild.CHECKS)
    assert len(NAMES) == 12
    for name, (src, _, _, _) in mbuild.CHECKS.items():
        assert src == name + ".cpp"


@pytest.mark.parametrize("name", NAMES)
def test_build_sees_the_files(name):
    src, hdrs, min_checks, _ = mbuild.CHECKS[name]
    srcp = os.path.join(CSRC, "host", src)
    assert os.path.exists(srcp)
    assert os.path.join(CSRC, "host", "check.hpp") in mbuild.check_headers(name)
    for h in mbuild.check_headers(name):
        assert os.path.exists(h), h
        assert h in mbuild.HEADERS or h in mbuild.HOST_HEADERS, h
    # every project header the source itself includes is listed
    for inc in re.findall(r'#include\s+"([^"]+)"', open(srcp).read()):
        assert os.path.normpath(os.path.join(CSRC, "host", inc)) in mbuild.check_headers(name), inc
    assert min_checks > 0


def test_build_leaves_the_programs():
    assert os.path.join(CSRC, "read_names_plan.hpp") in mbuild.HEADERS
    mbuild.build()
    for name in NAMES:
        assert os.access(os.path.join(mbuild.BIN, name), os.X_OK), name


@pytest.mark.parametrize("name", NAMES)
def test_check_program_runs(name):
    assert plain_checks(name) >= mbuild.CHECKS[name][2]


@pytest.mark.parametrize("name", NAMES)
def test_check_program_under_the_host_sanitizers(name, sanitized):
    n, stderr = run(sanitized[name], name)
    assert n == plain_checks(name) and n >= mbuild.CHECKS[name][2]
    assert "runtime error" not in stderr and "AddressSanitizer" not in stderr


def test_the_header_is_plain_cxx():
    """No HIP header, nothing but <cstdint>: what lets a host program and a device translation unit share it."""
    src = open(os.path.join(CSRC, "read_names_plan.hpp")).read()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)", src) == ["cstdint"]


def test_the_harness_is_plain_cxx():
    src = open(os.path.join(CSRC, "host", "check.hpp")).read()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)", src) == ["cstdio"]
