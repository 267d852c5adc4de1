"""SAM output without a GPU: the Python model of tests/sam_cases.py is held to results.txt through an
inverse that was written independently of it -- on every seeded case against the oracle's columns 1-3, and on the
reference's five fixtures against result_e.txt --, NM to the oracle's nmiss wherever the span is whole, the seeded cases
to the coverage they are there for, and the host function (musc::sam_text, the format's C++ copy) to the model byte for
byte through a small stand-alone program."""
import json
import os
import re
import subprocess

import pytest

from oracle import muscato_oracle as orc

import sam_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sc.seeded_cases()
REFUSALS = sc.refusal_cases()


def fields(record):
    f = record[:-1].split(b"\t")
    tags = dict((t[:2], t[5:]) for t in f[11:])
    return f, tags


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_inverse_recovers_the_oracle_columns(case):
    """Header + record -> (read, targetsub, pos) of every line of the oracle's results.txt, in its order; NM is the
    oracle's nmiss wherever the span is the whole read."""
    hdr, recs = sc.sam_of(case)
    cols = sc.oracle_columns(case)
    assert len(recs) == len(cols) > 0
    whole = 0
    for rec, (read, sub, pos, nmiss) in zip(recs, cols):
        assert sc.invert(hdr, rec)[:3] == (read, sub, pos), rec
        f, tags = fields(rec)
        assert int(tags[b"XM"]) == nmiss
        if len(sub) == len(read):
            assert int(tags[b"NM"]) == nmiss, rec
            whole += 1
    assert whole > 0


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_records_are_well_formed(case):
    """Eleven mandatory fields, the tags in their order, MD between two numbers with a 0 between adjacent letters, NH
    records per read numbered 1..NH by HI, the first of them primary, CIGAR as long as SEQ."""
    hdr, recs = sc.sam_of(case)
    ln = sc.parse_header(hdr)
    left, want = 0, 0  # records still due in the run of the read in hand, and its NH
    for rec in recs:
        assert rec.count(b"\n") == 1 and rec.endswith(b"\n")
        f, tags = fields(rec)
        assert len(f) in (16, 17) and [t[:5] for t in f[11:16]] == [b"NM:i:", b"MD:Z:", b"NH:i:", b"HI:i:", b"XM:i:"]
        assert len(f) == 16 or f[16].startswith(b"XC:i:")
        assert f[4] == b"255" and f[6:9] == [b"*", b"0", b"0"] and f[10] == b"*"
        assert re.fullmatch(rb"\d+([ACGTN]\d+)*", tags[b"MD"]), rec
        assert re.fullmatch(rb"[!-~]{1,254}", f[0]) and f[2] in ln and 1 <= int(f[3]) <= ln[f[2]] + 1
        assert tags[b"NM"] == b"%d" % len(re.findall(rb"[ACGTN]", tags[b"MD"]))
        if f[5] != b"*":
            assert sum(int(n) for n in re.findall(rb"(\d+)[MS]", f[5])) == len(f[9])
        hi, nh, flag = int(tags[b"HI"]), int(tags[b"NH"]), int(f[1])
        if left == 0:
            left = want = nh
        assert nh == want and hi == want - left + 1 and bool(flag & 256) == (hi != 1) and not flag & ~(16 | 256)
        left -= 1
    assert left == 0


def test_the_cases_cover_what_they_are_there_for():
    """Asserted from the data of the cases, not from their construction."""
    recs = {c.name: sc.sam_of(c)[1] for c in CASES}
    by = {c.name: c for c in CASES}
    # read lengths, and spans starting at every phase of a database word, at more than one stride of the read records
    strides = set()
    for name in ("lengths_33", "lengths_65", "lengths_130", "lengths_200"):
        c = by[name]
        lens = {len(r) for r in c.reads}
        assert lens >= {L for L in sc.LENS if L <= max(lens)}
        starts = [0]
        for t in c.targets:
            starts.append(starts[-1] + len(t))
        assert {(starts[g] + p) % 16 for _, g, p, _ in c.hits} == set(range(16))
        strides.add((max(lens) + 15) // 16 + 1)  # words of a record: the bases and the length word
    assert len(strides) == 4 and {len(r) for r in by["lengths_130"].reads} >= set(sc.LENS)
    # mismatches at the first and last base, adjacent, none, all; runs of 9, 10, 99 and 100
    mds = [fields(r)[1][b"MD"] for r in recs["mismatch_patterns"]]
    nums = {int(n) for md in mds for n in re.findall(rb"\d+", md)}
    assert {9, 10, 99, 100} <= nums
    assert any(re.fullmatch(rb"0[ACGT]\d+", md) for md in mds) and any(re.fullmatch(rb"\d+[ACGT]0", md) for md in mds)
    assert any(re.search(rb"[ACGT]0[ACGT]0[ACGT]", md) for md in mds) and any(re.fullmatch(rb"\d+", md) for md in mds)
    assert any(re.fullmatch(rb"(0[ACGT]){23}0", md) for md in mds)
    flags = {int(fields(r)[0][1]) & 16 for r in recs["mismatch_patterns"]}
    assert flags == {0, 16}
    # X in the read, in the database, at the same place in both
    cx = by["x"]
    kinds = set()
    for r, g, p, _ in cx.hits:
        for a, b in zip(cx.reads[r], cx.targets[g][p:]):
            kinds.add((a == ord("X"), b == ord("X")))
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}
    assert any(b"N" in fields(r)[1][b"MD"] for r in recs["x"]) and any(b"N" in fields(r)[0][9] for r in recs["x"])
    # clipped spans on both strands, and the empty span
    cig = {(int(fields(r)[0][1]) & 16, re.sub(rb"\d+", b"", fields(r)[0][5])) for r in recs["clipped"]}
    assert cig >= {(0, b"MS"), (16, b"SM"), (0, b"*"), (16, b"*")}
    # 1, 2 and 11 lines per read; genes without an id line
    assert {int(fields(r)[1][b"NH"]) for r in recs["lines_per_read"]} == {1, 2, 11}
    assert by["lines_per_read"].absent and len(recs["lines_per_read"]) < len(by["lines_per_read"].hits)
    assert all(b"XC" not in fields(r)[1] and fields(r)[0][0] == b"*" for r in recs["no_read_text"])
    # names
    tails = by["names"].tails
    for w in sc.WS:
        assert any(t.split(b"\t", 1)[1:] and bytes([w]) in t.split(b"\t", 1)[1] for t in tails)
    assert any(b";" in t for t in tails) and any(b"\t@" in t for t in tails) and any(b"\t>" in t for t in tails)
    assert any(len(t) > 300 for t in tails) and any(t.endswith(b"\t") for t in tails) and any(b"\t" not in t for t in tails)
    qn = {fields(r)[0][0] for r in recs["names"]}
    assert {b"*", b"plain", b"n1", b"at_name", b"gt_name", b"@two", b"A" * 254, b"B" * 254, b"C" * 254, b"w"} <= qn
    xc = {fields(r)[1].get(b"XC") for r in recs["names"]}
    assert {None, b"1", b"12", b"1234567", b"007"} <= xc and b"x9" not in xc
    assert {fields(r)[0][2] for r in recs["names"]} == {b"chr1", b"chr2", b"chr3", b">odd"}
    # rev_pairs with a pair without id lines: neither strand is in the header
    assert sc.parse_header(sc.sam_of(by["rev_absent"])[0]).keys() == {b"p0", b"p2"}


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: c.name)
def test_the_model_refuses(case):
    with pytest.raises(sc.SamRefused):
        sc.sam_of(case)
    if case.rev_pairs and case.name in ("odd_count", "unequal_pair", "even_partner_absent"):
        case.rev_pairs = False  # the same inputs are fine without the pairing
        try:
            assert len(sc.sam_of(case)[1]) <= 1
        finally:
            case.rev_pairs = True


# ------------------------------------------------------------------------------------------------- the reference's fixtures
FIXTURES = [("00", False, False), ("01", False, False), ("02", False, False), ("03", False, False), ("04", True, False),
            ("04", True, True)]


def fixture_case(golden_dir, case, rev, rev_pairs):
    d = os.path.join(golden_dir, "muscato", case)
    rd = lambda n: open(os.path.join(d, n), "rb").read()
    cfg = orc.Config.from_json(json.loads(rd("config.json")))
    targets, ids = orc.prep_targets_file(os.path.join(d, "genes.txt"), rev)
    ureads = orc.uniqify(orc.prep_reads(orc.read_fastq(rd("reads.fastq")), cfg))
    rests = [i.split(b"\t", 1)[1] for i in ids]
    num = {u.seq: i for i, u in enumerate(ureads)}
    lines = [ln.split(b"\t") for ln in rd("result_e.txt").split(b"\n")[:-1]]
    hits = [(num[c[0]], rests.index(c[4] + b"\t" + c[5]), int(c[2]), int(c[3])) for c in lines]
    tails = [b"%d\t%s" % (u.count, u.names) for u in ureads]
    c = sc.Case("fixture_" + case, [u.seq for u in ureads], targets, rests, hits, tails, (), rev_pairs)
    return c, lines


@pytest.mark.parametrize("case,rev,rev_pairs", FIXTURES)
def test_fixture_round_trip(golden_dir, case, rev, rev_pairs):
    """The lines of result_e.txt, in the file's own order, through the model and back through the inverse: columns 1-3,
    and the gene name with its `_r` on the reverse strand."""
    c, lines = fixture_case(golden_dir, case, rev, rev_pairs)
    hdr = sc.header(c.targets, c.rests, (), rev_pairs)
    recs = sc.records(c.reads, c.targets, c.rests, c.tails, c.hits, rev_pairs)
    assert len(recs) == len(lines) > 0
    for rec, col in zip(recs, lines):
        assert sc.invert(hdr, rec) == (col[0], col[1], int(col[2]), col[4]), rec
        f, tags = fields(rec)
        assert int(tags[b"NM"]) == int(col[3]) and tags[b"XC"] == col[6]
        assert f[0] == col[7].lstrip(b">@").split(b";")[0]
    if rev_pairs:
        assert any(int(fields(r)[0][1]) & 16 for r in recs) and not any(k.endswith(b"_r") for k in sc.parse_header(hdr))
    elif rev:
        assert any(k.endswith(b"_r") for k in sc.parse_header(hdr))


# ------------------------------------------------------------------------------------------------------ the host function
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sam_driver") / "sam_host_driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "sam_host_driver.cpp")])
    return exe


def driver_input(case):
    h = lambda s: b"h" + s.hex().encode()
    ordered = sc.ordered_hits(case)
    out = [b"%d %d %d %d %d" % (case.rev_pairs, case.tails is not None, len(case.reads), len(case.targets), len(ordered))]
    out += [h(r) for r in case.reads]
    out += [h(t) for t in case.tails or []]
    out += [h(t) for t in case.targets]
    out += [b"-" if g in case.absent else h(r) for g, r in enumerate(case.rests)]
    out += [b"%d %d %d %d" % tuple(x) for x in ordered]
    return b"\n".join(out) + b"\n"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_host_function_equals_the_model(driver, case):
    r = subprocess.run([driver], input=driver_input(case), capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr
    hdr, recs = sc.sam_of(case)
    assert r.stdout == hdr + b"".join(recs)


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: c.name)
def test_host_function_refuses(driver, case):
    r = subprocess.run([driver], input=driver_input(case), capture_output=True, timeout=60)
    assert r.returncode == 12 and r.stdout == b"" and len(r.stderr) > 0
