"""Coverage without a GPU: the brute-force model of tests/cov_cases.py is held two independent ways -- to
a depth count made from the SAM model's records of the same list (POS, the M length of CIGAR, XC, NH) and to one made
from the lines of results.txt (the oracle's on the seeded cases, result_e.txt on the reference's five fixtures) --, the
seeded cases to what they are there for, and the host function (musc::coverage_text, the stage's C++ copy) to the model
byte for byte through a small stand-alone program."""
import os
import re
import subprocess

import pytest

from oracle import muscato_oracle as orc

import cov_cases as cc
import sam_cases as sc
from test_sam_cases import FIXTURES, fixture_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cc.seeded_cases()
REFUSALS = cc.refusal_cases()
RUNS = [(c, f) for c in CASES for f in c.flagsets if f not in c.refused]
REFUSED_RUNS = [(c, f) for c in CASES + REFUSALS for f in c.refused]
run_id = lambda v: v.name if isinstance(v, cc.CovCase) else "".join("rwu"[i] if b else "-" for i, b in enumerate(v))


def parse(bed, summary):
    """({name: [(start, end, depth)]}, {name: (len, numreads, covbases, sumdepth, maxdepth)}) of the two texts."""
    runs, stats = {}, {}
    for rec in bed:
        assert re.fullmatch(rb"[!-~]+\t\d+\t\d+\t[1-9]\d*\n", rec), rec
        name, s, e, d = rec[:-1].split(b"\t")
        runs.setdefault(name, []).append((int(s), int(e), int(d)))
    for rec in summary:
        assert re.fullmatch(rb"[!-~]+(\t\d+){5}\n", rec), rec
        f = rec[:-1].split(b"\t")
        assert f[0] not in stats
        stats[f[0]] = tuple(int(v) for v in f[1:])
    return runs, stats


def from_differences(lengths, pieces):
    """The same two dicts from a difference array per name: pieces = [(name, a, S, w)], lengths = {name: len}."""
    diff = {n: [0] * (l + 1) for n, l in lengths.items()}
    numreads = dict.fromkeys(lengths, 0)
    for name, a, S, w in pieces:
        numreads[name] += w
        if S:
            diff[name][a] += w
            diff[name][a + S] -= w
    runs, stats = {}, {}
    for name, dd in diff.items():
        depth, start, out, cov, area, top = 0, 0, [], 0, 0, 0
        for x, delta in enumerate(dd):
            if not delta:
                continue
            if depth:
                out.append((start, x, depth))
                cov, area, top = cov + x - start, area + (x - start) * depth, max(top, depth)
            depth, start = depth + delta, x
        assert depth == 0
        if out:
            runs[name] = out
        stats[name] = (lengths[name], numreads[name], cov, area, top)
    return runs, stats


@pytest.mark.parametrize("case,flags", RUNS, ids=run_id)
def test_model_equals_a_count_from_the_sam_records(case, flags):
    """POS, the M length of CIGAR, XC and NH of the SAM model's records of the same ordered list."""
    rev_pairs, weighted, unique = flags
    c = case.case
    ordered = sc.ordered_hits(c)
    hdr = sc.header(c.targets, c.rests, c.absent, rev_pairs)
    recs = sc.records(c.reads, c.targets, c.rests, c.tails, ordered, rev_pairs, c.absent)
    lengths = sc.parse_header(hdr)
    pieces = []
    for rec in recs:
        f = rec[:-1].split(b"\t")
        tags = dict((t[:2], t[5:]) for t in f[11:])
        if unique and tags[b"NH"] != b"1":
            continue
        m = re.search(rb"(\d+)M", f[5])
        w = min(int(tags[b"XC"]), cc.WEIGHT_LIMIT) if weighted and b"XC" in tags else 1
        pieces.append((f[2], int(f[3]) - 1, int(m.group(1)) if m else 0, w))
    assert parse(*cc.cov_of(c, ordered, *flags)) == from_differences(lengths, pieces)


def simple_rests(c):
    """Every gene text is `name<TAB>len` with the name its own RNAME token: column 5 of results.txt names the target."""
    return all(r.count(b"\t") == 1 and r.split(b"\t")[0] == sc.rname_of(r) for r in c.case.rests)


@pytest.mark.parametrize("case", [c for c in CASES if simple_rests(c)], ids=run_id)
def test_model_equals_a_count_from_the_oracles_results(case):
    """Columns 1, 2, 3 and 5 of the oracle's results.txt: a line covers [pos, pos + len(targetsub)) of the gene it names;
    with the unique flag only the lines whose read is on no other line."""
    c = case.case
    ids = [b"%011d\t%s" % (g, c.rests[g]) for g in range(len(c.targets))]
    kept = [tuple(int(v) for v in h) for h in c.hits if int(h[1]) not in c.absent]
    txt = orc.results_text(kept, [orc.UniqueRead(r, 1, b"n") for r in c.reads], c.targets, ids, orc.Config(MMTol=sc.KEEP_ALL))
    cols = [ln.split(b"\t") for ln in txt.split(b"\n")[:-1]]
    assert [(col[0], col[1], int(col[2]), int(col[3])) for col in cols] == sc.oracle_columns(c)
    lengths = {sc.rname_of(c.rests[g]): len(c.targets[g]) for g in range(len(c.targets)) if g not in c.absent}
    assert len(lengths) == len(c.targets) - len(c.absent)  # (the names of a case are distinct)
    per_read = {}
    for col in cols:
        per_read[col[0]] = per_read.get(col[0], 0) + 1
    for unique in (False, True):
        pieces = [(sc.rname_of(col[4]), int(col[2]), len(col[1]), 1) for col in cols if not unique or per_read[col[0]] == 1]
        assert parse(*cc.cov_of(c, sc.ordered_hits(c), False, False, unique)) == from_differences(lengths, pieces)


@pytest.mark.parametrize("case,rev,rev_pairs", FIXTURES)
def test_fixture_counts(golden_dir, case, rev, rev_pairs):
    """The lines of result_e.txt: name, pos, the length of targetsub and the count column; a line of an `_r` gene is
    folded by hand when the pairs are."""
    c, lines = fixture_case(golden_dir, case, rev, rev_pairs)
    lengths = {sc.rname_of(r): len(t) for g, (r, t) in enumerate(zip(c.rests, c.targets)) if not (rev_pairs and g % 2)}
    per_read = {}
    for col in lines:
        per_read[col[0]] = per_read.get(col[0], 0) + 1
    for weighted, unique in ((False, False), (True, False), (False, True), (True, True)):
        pieces = []
        for col in lines:
            if unique and per_read[col[0]] != 1:
                continue
            name, pos, S = col[4], int(col[2]), len(col[1])
            if rev_pairs and name.endswith(b"_r"):
                name, pos = name[:-2], int(col[5]) - pos - S
            pieces.append((name, pos, S, int(col[6]) if weighted else 1))
        got = parse(*cc.cov_of(c, c.hits, rev_pairs, weighted, unique))
        assert got == from_differences(lengths, pieces) and got[0]
    if rev_pairs:
        assert any(col[4].endswith(b"_r") for col in lines)


def test_the_cases_cover_what_they_are_there_for():
    """Asserted from the data of the cases and the model's texts, not from their construction."""
    by = {c.name: c for c in CASES}
    out = lambda name, flags: parse(*cc.cov_case_of(by[name], flags))
    # abutting intervals: one run when the weights are equal, two when they are not; nested and identical intervals
    runs, _ = out("intervals", cc.WEIGHTED)
    assert runs[b"abut_eq"] == [(10, 50, 3)] and runs[b"abut_ne"] == [(10, 30, 2), (30, 50, 5)]
    assert runs[b"nested"] == [(60, 70, 1), (70, 80, 5), (80, 100, 1)] and runs[b"same"] == [(5, 30, 18)]
    assert out("intervals", cc.PLAIN)[0][b"abut_ne"] == [(10, 50, 1)]
    # many events on one key
    c = by["piles"].case
    starts = {}
    for _, g, pos, _ in c.hits:
        starts[(g, pos)] = starts.get((g, pos), 0) + 1
    assert sorted(starts.values()) == sorted(cc.PILES)
    assert {s[4] for s in out("piles", cc.PLAIN)[1].values()} == set(cc.PILES)
    # target ends
    c = by["target_ends"].case
    runs, stats = out("target_ends", cc.PLAIN)
    assert runs[b"e0"][-1][1] == len(c.targets[0]) and runs[b"e2"][0][0] == 0 and len(c.targets[1]) == 0
    assert runs[b"e2"][-1][1] == len(c.targets[2]) and runs[b"e3"] == [(0, 30, 1)]
    assert [len(t) for t in c.targets].count(0) == 3 and stats[b"e1"] == (0, 0, 0, 0, 0) and stats[b"e4"] == (0, 0, 0, 0, 0)
    assert stats[b"e6"][1:] == (0, 0, 0, 0) and stats[b"e7"][1:] == (0, 0, 0, 0) and b"e6" not in runs
    assert b"e0" in runs and b"e9" in runs and runs[b"e9"][-1][1] == len(c.targets[9])
    assert b"e5" not in stats and b"e8" not in stats and any(g == 5 for _, g, _, _ in c.hits) and len(stats) == 8
    # clipped spans, S == 0, both strands over the same bases
    c = by["strands"].case
    spans = [cc.interval_of(c.targets, g, p, len(c.reads[r]), True) + (g % 2, len(c.reads[r])) for r, g, p, _ in c.hits]
    assert {(S == 0, rev) for _, _, S, rev, _ in spans} >= {(True, 0), (True, 1)}
    assert {rev for _, _, S, rev, L in spans if 0 < S < L} == {0, 1}
    fwd = {(f, a, S) for f, a, S, rev, _ in spans if not rev and S}
    assert any((f, a, S) in fwd for f, a, S, rev, _ in spans if rev)
    folded, plain = out("strands", cc.REV), out("strands", cc.PLAIN)
    assert set(folded[1]) == {b"s0", b"s1"} and set(plain[1]) == {b"s0", b"s0_r", b"s1", b"s1_r"}
    assert folded[1][b"s0"][1] == plain[1][b"s0"][1] + plain[1][b"s0_r"][1]
    assert by["clipped"].case.rev_pairs and parse(*cc.cov_case_of(by["clipped"], (True, False, False)))[0]
    # weights
    c = by["weights"]
    heads = {t.split(b"\t", 1)[0] for t in c.note["tail_list"]}
    assert {b"0", b"1", b"12345", b"007", b"x9", b"", b"42", b"nocount"} <= heads and any(b"\t" not in t for t in c.note["tail_list"])
    runs, stats = out("weights", cc.WEIGHTED)
    depths = {d for r in runs.values() for _, _, d in r}
    assert {1, 12345, 7, 42, 6} <= depths and 0 not in depths
    assert stats[b"w"][1] == 0 + 1 + 12345 + 7 + 1 + 1 + 1 + 42 + 1 + 1 + 1 + 1 + 0 + 6 + 6
    assert out("weights", cc.PLAIN)[1][b"w"][1] == len(c.case.hits) == 15
    assert out("weights", (False, True, True))[1][b"w"][1] == stats[b"w"][1] - 12
    assert by["cov_no_read_text"].case.tails is None and out("cov_no_read_text", cc.WEIGHTED) == out("weights", cc.PLAIN)
    # the totals on either side of 2^32, and a count of eleven digits
    assert out("total_max", cc.WEIGHTED)[1][b"big"][1] == (1 << 32) - 1
    assert max(d for _, _, d in out("total_max", cc.WEIGHTED)[0][b"big"]) == (1 << 32) - 1
    for name in ("total_over", "eleven_digits"):
        with pytest.raises(cc.CovRefused):
            cc.cov_case_of(by[name], cc.WEIGHTED)
        assert out(name, cc.PLAIN)[0]
    assert any(len(t.split(b"\t")[0]) == 11 for t in by["eleven_digits"].case.tails)
    # decimal widths
    runs, stats = out("widths", cc.WEIGHTED)
    assert {len(str(d)) for _, _, d in runs[b"deep"]} == set(range(1, 11))
    assert {d for _, _, d in runs[b"deep"]} == set(by["widths"].note["depths"])
    for w in cc.WIDTHS:
        assert any(s == w for s, _, _ in runs[b"long"]) and any(e == w + (w % 10 == 9) for _, e, _ in runs[b"long"]), w
    assert {len(str(s)) for s, _, _ in runs[b"long"]} == set(range(1, 7)) and stats[b"long"][0] == 100005 and runs[b"long"][-1][1] == 100005
    assert any(s > 65535 for s, _, _ in runs[b"long"])
    # uniqueness
    c = by["unique"]
    lines = {}
    for r, _, _, _ in c.case.hits:
        lines[r] = lines.get(r, 0) + 1
    assert sorted(lines.values()) == [1, 1, 2, 3]
    assert sum(s[1] for s in out("unique", cc.UNIQUE)[1].values()) == 2 and sum(s[1] for s in out("unique", cc.PLAIN)[1].values()) == 7
    assert sum(s[1] for s in out("unique", (False, True, True))[1].values()) == 5
    # list sizes
    assert [len(by["list_%d" % n].case.hits) for n in (0, 1, 64, 65, 257)] == [0, 1, 64, 65, 257]
    assert cc.cov_case_of(by["list_0"], cc.PLAIN) == ([], [b"l0\t400\t0\t0\t0\t0\n", b"l1\t30\t0\t0\t0\t0\n"])


@pytest.mark.parametrize("case,flags", REFUSED_RUNS, ids=run_id)
def test_the_model_refuses(case, flags):
    with pytest.raises(cc.CovRefused):
        cc.cov_case_of(case, flags)


# ------------------------------------------------------------------------------------------------------ the host function
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cov_driver") / "cov_host_driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cov_host_driver.cpp")])
    return exe


def driver_input(c, flags):
    h = lambda s: b"h" + s.hex().encode()
    ordered = sc.ordered_hits(c)
    bits = (1 if flags[0] else 0) | (2 if flags[1] else 0) | (4 if flags[2] else 0)
    out = [b"%d %d %d %d %d" % (bits, c.tails is not None, len(c.reads), len(c.targets), len(ordered))]
    out += [h(r) for r in c.reads]
    out += [h(t) for t in c.tails or []]
    out += [h(t) for t in c.targets]
    out += [b"-" if g in c.absent else h(r) for g, r in enumerate(c.rests)]
    out += [b"%d %d %d %d" % tuple(x) for x in ordered]
    return b"\n".join(out) + b"\n"


@pytest.mark.parametrize("case,flags", RUNS, ids=run_id)
def test_host_function_equals_the_model(driver, case, flags):
    r = subprocess.run([driver], input=driver_input(case.case, flags), capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr
    bed, summary = cc.cov_case_of(case, flags)
    assert r.stdout == b"".join(bed) + b"#summary\n" + b"".join(summary)


@pytest.mark.parametrize("case,flags", REFUSED_RUNS, ids=run_id)
def test_host_function_refuses(driver, case, flags):
    r = subprocess.run([driver], input=driver_input(case.case, flags), capture_output=True, timeout=60)
    assert r.returncode == 12 and r.stdout == b"" and len(r.stderr) > 0
