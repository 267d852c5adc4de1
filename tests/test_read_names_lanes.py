"""What a lane of the read-name stage computes (muscato_amd/csrc/read_names_lanes.hpp), without a GPU:
the header is plain C++ that g++ compiles without HIP, it holds no cross-lane primitive and no loop without a constant
bound, and host/read_names_plan_check.cpp -- one of the twelve check programs, built and run plain and under the
sanitizers by tests/test_check_programs.py -- runs every item function of it in lock step against the reference's
string code."""
import os
import re
import subprocess

from muscato_amd import build as mbuild

import abi_header as ah

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muscato_amd", "csrc")
LANES = os.path.join(CSRC, "read_names_lanes.hpp")
CHECK = os.path.join(CSRC, "host", "read_names_plan_check.cpp")


def code(path):
    """The file without its comments."""
    src = open(path).read()
    return ah.strip_comments(src, line_comments=True)


def test_the_header_is_plain_cxx_and_listed():
    src = open(LANES).read()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)", src) == ["cstdint", "read_names_plan.hpp"]
    assert LANES in mbuild.HEADERS
    assert LANES in mbuild.check_headers("read_names_plan_check")
    assert mbuild.CHECKS["read_names_plan_check"][2] >= 21_627_000  # (the size rules alone were 21 577 989)


def test_no_cross_lane_primitive():
    src = code(LANES)
    for word in ("__shfl", "__ballot", "__any", "__all", "__syncthreads", "__shared__", "readfirstlane", "readlane", "atomic", "__activemask",
                 "__builtin_amdgcn", "threadIdx", "blockIdx", "__global__", "hip/"):
        assert word not in src, word


def test_every_loop_has_a_constant_bound():
    """for (init; i < BOUND; step) with BOUND a literal or a constant of the plan -- the data may only end a loop sooner
    -- but for the dword loop of the store, which strides by the wave over a length that is an argument."""
    src = code(LANES)
    assert "while" not in src and "goto" not in src
    loops = re.findall(r"for\s*\(([^;]*);([^;]*);([^)]*)\)", src)
    assert len(loops) >= 7
    bounds = {"8", "10", "CMP_WORDS", "NAME_LIMIT", "WAVE_GROUP_MAX", "JOIN_SCAN_MAX", "SEARCH_STEPS"}
    by_argument = 0
    for init, cond, step in loops:
        m = re.fullmatch(r"\s*(\w+)\s*<\s*(\w+)\s*", cond)
        assert m, cond
        if m.group(2) in bounds:
            continue
        assert (m.group(1), m.group(2), step.strip()) == ("d", "nd", "d += 64"), (init, cond, step)
        by_argument += 1
    assert by_argument == 1
    consts = dict(re.findall(r"constexpr uint32_t (\w+) = ([^;]+);", open(LANES).read()))
    assert consts["CMP_WORDS"].startswith("(NAME_KEEP + DOTS + 7) / 8") and consts["JOIN_SCAN_MAX"].startswith("JOIN_LIMIT + 2")


def test_the_check_program_runs_every_item_function():
    items = set(re.findall(r"\b(\w+_item)\s*\(", code(LANES)))
    assert items == {"measure_item", "rank_item", "pairs_item", "unpairs_item", "sizes_item", "record_item", "copy_item", "line_item"}
    check = code(CHECK)
    for fn in sorted(items) + ["PairLess", "CheckedText", "loads_outside == 0"]:
        assert fn in check, fn


def test_lock_step_part_counts():
    """The program built by build(): more checks than the size rules alone gave, and nothing on stderr."""
    exe = mbuild.build_checks()["read_names_plan_check"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    n = int(re.fullmatch(r"read_names_plan_check: (\d+) checks passed\n", r.stdout).group(1))
    assert n >= mbuild.CHECKS["read_names_plan_check"][2] > 21_577_989
