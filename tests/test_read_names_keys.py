"""The order of the larger groups of the read-name stage as integer keys (muscato_amd/csrc/read_names_keys.hpp,
DESIGN.md 23), without a GPU: the header is plain C++ that g++ compiles alone, the check program watches it, its code
holds no cross-lane primitive and no open loop, no file of the stage names a comparator-driven library sort, and the
W + 2 stable key passes, restated here over the model's name_word, order the larger groups of every case as the model's
comparison sort does -- whatever the order in which the pairs enter."""
import os
import random
import re
import subprocess

import pytest

from muscato_amd import build as mbuild

import abi_header as ah
import read_names_cases as rn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muscato_amd", "csrc")
KEYS = os.path.join(CSRC, "read_names_keys.hpp")
CMP_WORDS = (rn.NAME_KEEP + rn.DOTS + 7) // 8


def code(path):
    """The file without its comments."""
    src = open(path).read()
    return ah.strip_comments(src, line_comments=True)


def test_the_header_is_plain_cxx_and_listed(tmp_path):
    assert re.findall(r"#include\s+[<\"]([^>\"]+)", open(KEYS).read()) == ["cstdint", "read_names_lanes.hpp"]
    assert KEYS in mbuild.HEADERS
    assert KEYS in mbuild.check_headers("read_names_plan_check")
    assert mbuild.CHECKS["read_names_plan_check"][2] >= 21_928_502  # (21 627 000 before the key passes)
    tu = tmp_path / "keys.cpp"
    tu.write_text('#include "%s"\nint main() { return musc_rn::key_passes(0) == 2 && musc_rn::key_passes(2000) == %d ? 0 : 1; }\n'
                  % (KEYS, CMP_WORDS + 2), encoding="ascii")
    exe = str(tmp_path / "keys")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, str(tu)])
    assert subprocess.run([exe]).returncode == 0


def test_no_cross_lane_primitive_and_no_open_loop():
    src = code(KEYS)
    for word in ("__shfl", "__ballot", "__any", "__all", "__syncthreads", "__shared__", "readfirstlane", "readlane", "atomic", "__activemask",
                 "__builtin_amdgcn", "threadIdx", "blockIdx", "__global__", "hip/", "while", "goto", "_item"):
        assert word not in src, word
    loops = re.findall(r"for\s*\(([^;]*);([^;]*);([^)]*)\)", src)
    for _, cond, _ in loops:
        assert re.fullmatch(r"\s*\w+\s*<\s*GROUP_STEPS\s*", cond), cond
    assert "constexpr uint32_t GROUP_STEPS = 32;" in src


def test_no_file_of_the_stage_names_a_comparator_sort():
    stage = [p for p in mbuild.HEADERS + mbuild.SOURCES if "read_names" in os.path.basename(p)]
    assert KEYS in stage and len(stage) >= 4
    for p in stage:
        assert "merge_sort" not in open(p).read(), p


# ---- the key passes, restated
def key_words(max_clip):
    return min((max_clip + 7) // 8, CMP_WORDS)


def by_keys(pairs, names, entry):
    """pairs: (group, kept read); entry: the order in which they enter.  Stable passes, the least significant first."""
    W = key_words(max(rn.clipped_len(len(names[y])) for _, y in pairs))
    cur = [pairs[k] for k in entry]
    cur.sort(key=lambda p: rn.clipped_len(len(names[p[1]])) << 32 | p[1])  # (list.sort is stable)
    for w in reversed(range(W)):
        cur.sort(key=lambda p: rn.name_word(names[p[1]], w))
    cur.sort(key=lambda p: p[0])
    return cur, W


@pytest.mark.parametrize("case", rn.cases(), ids=lambda c: c.name)
def test_key_passes_order_the_larger_groups_as_the_model_does(case):
    m = rn.model_of(case)
    names = m.prep.names
    want = [(g, y) for g, mem in enumerate(m.members) if len(mem) > rn.WAVE_GROUP_MAX for y in mem]
    if not want:
        assert m.info["n_sorted_groups"] == 0
        return
    pairs = sorted(want, key=lambda p: (p[0], p[1]))  # as the stage makes them: group by group, file order
    rng = random.Random(len(pairs))
    shuffled = list(range(len(pairs)))
    rng.shuffle(shuffled)
    for entry in (list(range(len(pairs))), list(reversed(range(len(pairs)))), shuffled):
        got, W = by_keys(pairs, names, entry)
        assert got == want
        assert W == key_words(max(rn.clipped_len(len(names[y])) for _, y in want))


def test_cases_reach_the_word_counts_and_sizes():
    """Among the cases: a larger group of empty names (W = 0), one of exactly 65, and the 3 198 pairs of `counts`."""
    by_name = {c.name: rn.model_of(c) for c in rn.cases() if c.name in ("counts", "group_sizes")}
    counts = by_name["counts"]
    big = [mem for mem in counts.members if len(mem) > rn.WAVE_GROUP_MAX]
    assert sorted(len(mem) for mem in big) == [99, 100, 999, 1000, 1000] and sum(len(mem) for mem in big) == 3198
    assert any(all(len(counts.prep.names[y]) == 0 for y in mem) for mem in big)
    assert 65 in [len(mem) for mem in by_name["group_sizes"].members]
