"""The plain-C++ part of the read-name stage without a GPU: read_names_plan.hpp is seen by the build, and
read_names_plan_check -- the stand-alone program that holds it to the reference's string code -- is built by
muscato_amd/build.py, and built again with AddressSanitizer and UBSan and run."""
import os
import re
import subprocess

from muscato_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muscato_amd", "csrc")


def test_build_sees_the_new_files():
    assert os.path.join(CSRC, "read_names_plan.hpp") in mbuild.HEADERS
    assert "read_names_plan_check" in mbuild.CHECKS
    src, hdrs = mbuild.CHECKS["read_names_plan_check"]
    assert os.path.exists(os.path.join(CSRC, "host", src)) and all(os.path.exists(os.path.join(CSRC, h)) for h in hdrs)
    mbuild.build()
    assert os.access(os.path.join(mbuild.BIN, "read_names_plan_check"), os.X_OK)


def test_plan_check_program_runs():
    exe = mbuild.build_checks()["read_names_plan_check"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


def test_plan_check_program_under_the_host_sanitizers(tmp_path):
    """A program of its own with its own main: compiled with -fsanitize=address,undefined, the runtimes linked in."""
    exe = mbuild.build_checks(force=True, sanitize=True, out_dir=str(tmp_path))["read_names_plan_check"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"read_names_plan_check: (\d+) checks passed", r.stdout)
    assert m and int(m.group(1)) > 1000000
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_header_is_plain_cxx():
    """No HIP header, nothing but <cstdint>: what lets a host program and a device translation unit share it."""
    src = open(os.path.join(CSRC, "read_names_plan.hpp")).read()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)", src) == ["cstdint"]
