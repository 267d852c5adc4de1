"""The inputs of the long-read tests (tests/long_read_cases.py), checked without a GPU: the two CPU oracles agree on
every case -- beyond a few hundred bases they are the only pin -- and every case still holds, in the ORACLE's tuples,
what it exists for: a full-length read accepted at exactly its budget and its twin one mismatch over rejected, a read
flush with the database's last base and its overhanging twin, three- and four-digit nmiss, two placements further
apart than MMTol, the lengths where the budget rounds down."""
import numpy as np
import pytest

from oracle import muscato_oracle as orc

import loader_cases as lc
import long_read_cases as lr


def by_read(name):
    """read index -> [(gene, pos, nmiss)] of the case's oracle tuples."""
    out = {}
    for r, g, p, nx in lr.oracle_hits(name).tolist():
        out.setdefault(r, []).append((g, p, nx))
    return out


def test_shapes():
    assert tuple(lc.record_words(m) for m in lr.LMAXES) == (64, 68, 260, 4100)
    assert {s[0] for s in lr.SPECS.values()} == set(lr.LMAXES)
    assert {len(s[1]) for s in lr.SPECS.values() if s[0] == 4099} == {1, 2, 3}  # W2 true and false
    assert {s[2] for s in lr.SPECS.values()} == {0.9, 0.97}
    for lmax in (4099, 65535):
        assert {s[4] for s in lr.SPECS.values() if s[0] == lmax} == {"", "reads", "db"}
    assert lr.SPECS["L4099-far"][1] == (0, 4000) and lr.SPECS["L65535-far"][1] == (0, 65500)
    # words 64 and 65 are the first two a 1 000-base stride does not have; base 1 024 opens word 64
    assert lr.WORD64 // 16 == 64 and lr.WORD65 // 16 == 65 and lr.X_READ_PLACES[0] == 64 * 16
    assert lr.X_READ_PLACES[1] // 16 + 1 == lr.X_READ_PLACES[2] // 16 and lr.X_READ_PLACES[2] % 16 == 0


def test_budget_rounding():
    """1 - 0.9 is 0.09999999999999998 in IEEE double: a length that is a multiple of ten has budget L / 10 - 1."""
    assert 1 - 0.9 == 0.09999999999999998
    tens = [n for n in range(256, 65536) if n % 10 == 0]
    assert len(tens) == 6528 and all(lr.budget(0.9, n) == n // 10 - 1 for n in tens)
    assert [lr.budget(0.9, n) for n in (1000, 4090, 65530, 65535)] == [99, 408, 6552, 6553]
    assert lr.budget(0.97, 1009) == 30 and lr.budget(0.97, 4099) == 122
    for p in (0.9, 0.97):
        for n in (lr.step_up(p, 258), lr.step_down(p, 65535)):
            assert lr.budget(p, n) == lr.budget(p, n - 1) + 1


@pytest.mark.parametrize("name", lr.NAMES)
def test_inputs(name):
    c = lr.case(name)
    assert c is lr.case(name)  # made once, shared
    assert c.reads == sorted(set(c.reads)) and max(map(len, c.reads)) == c.lmax
    assert [len(t) for t in c.targets] == [c.lmax + 300, c.lmax + 300, 500, 0, 180]
    t0, t0p = c.targets[0], c.targets[1]
    diff = [i for i in range(len(t0p)) if c.t0[i] != t0p[i]]
    assert diff == list(range(96, len(t0p), 97))
    assert all(len(c.read_of("ph%d_b" % (c.lmax - d))) == c.lmax - d for d in lr.PHASES[1:])
    assert {len(c.read_of("split%d_b" % n)) for n in lr.SPLIT_LENS} == {255, 256, 257}
    assert min(c.step_lens) > 257 and c.lmax - 40 < max(c.step_lens) <= c.lmax
    # mismatches from the last base backwards, in words 64 and 65, none inside a window
    r, span = c.read_of("long_b"), t0[lr.T0_AT:lr.T0_AT + c.lmax]
    mm = [i for i in range(c.lmax) if r[i] != span[i]]
    assert len(mm) == c.budget and mm[-1] == c.lmax - 1 and not set(mm) & c.inwin
    if c.lmax > 1056:
        assert any(i // 16 == 64 for i in mm) and any(i // 16 == 65 for i in mm)
    assert max(b - a for a, b in zip(mm, mm[1:])) <= 2 * c.lmax // max(1, c.budget) + 2 * lr.WW + 4  # spread out
    w0 = c.read_of("long_w0")
    assert [i for i in range(c.lmax) if w0[i] != c.read_of("long_0")[i]] == [5] and 5 < min(c.windows[1:] or [lr.WW])
    # the X variants
    xr = [i for i, b in enumerate(c.read_of("long_0")) if b == ord("X")]
    xt = [i - lr.T0_AT for i, b in enumerate(t0) if b == ord("X")]
    assert xr == {"": [], "reads": [1024, 2047, 2048, c.lmax - 1], "db": [2048]}[c.x]
    assert xt == ([1024, 2048, c.lmax - 1] if c.x == "db" else [])
    assert all(c.t0[lr.T0_AT + p] == ord("A") for p in xr + xt)  # only the mask plane tells an X from this base
    assert not (set(xr) | set(xt)) & c.inwin
    assert any(b == ord("X") for rd in c.reads for b in rd) == (c.x != "")


@pytest.mark.parametrize("name", lr.NAMES)
def test_the_oracles_agree(name):
    c = lr.case(name)
    direct = np.array(sorted(orc.match_direct(c.reads, c.targets, c.ocfg())), dtype=np.uint32).reshape(-1, 4)
    lit = lr.oracle_hits(name)
    assert direct.shape == lit.shape and (direct == lit).all()
    assert not lit.flags.writeable and lit is lr.oracle_hits(name)


@pytest.mark.parametrize("name", lr.NAMES)
def test_coverage(name):
    c = lr.case(name)
    hits = by_read(name)
    R = c.roles
    lens = [len(r) for r in c.reads]
    # accepted at exactly the budget, rejected one over it -- at full length and at every phase of the last word
    assert (0, lr.T0_AT, c.budget) in hits[R["long_b"]] and lens[R["long_b"]] == c.lmax
    assert (0, lr.T0_AT, c.budget - 1) in hits[R["long_bm1"]]
    assert R["long_bp1"] not in hits
    for n in c.phase_lens[1:] + c.step_lens + list(lr.SPLIT_LENS):
        tag = "split" if n in lr.SPLIT_LENS else "ph" if n in c.phase_lens else "step"
        at = 300 if tag == "split" else lr.T0_AT
        assert (0, at, lr.budget(c.pmatch, n)) in hits[R["%s%d_b" % (tag, n)]], (tag, n)
        assert R["%s%d_bp1" % (tag, n)] not in hits, (tag, n)
    # where the database ends
    for role, gene in (("flush_last_40", 4), ("flush_last_57", 4), ("flush_last_120", 4), ("flush_t0_40", 0), ("flush_t0_200", 0)):
        r = R[role]
        assert any(g == gene and p + lens[r] == len(c.targets[g]) and nx == 0 for g, p, nx in hits[r]), role
    ends = [sum(len(t) for t in c.targets[:g]) + p + lens[r] for r, hs in hits.items() for g, p, _ in hs]
    assert max(ends) == c.total_bases and ends.count(c.total_bases) == 3
    for role in ("over_last_40", "over_last_57", "straddle_t0", "straddle_mid"):
        assert R[role] not in hits, role
    db = b"".join(c.targets)
    assert c.read_of("straddle_t0") in db and c.read_of("straddle_mid") in db  # contiguous there, in no single target
    assert (c.read_of("over_last_40")[:-1] + b"A") == c.read_of("over_last_40") and db.endswith(c.read_of("over_last_40")[:-1])
    # position 0: window 0 places a read of at most 100 - q2 bases, a later window any
    assert hits[R["pos0_85_w0"]] == [(0, 0, 1), (1, 0, 1)]  # (T0' begins as T0 does)
    assert (R["pos0_86_w0"] in hits) == any(q > 25 and q + lr.WW <= 86 for q in c.windows)  # (its mismatch is base 25)
    later = any(20 <= q <= 120 - lr.WW for q in c.windows)
    assert (0, 0, 0) in hits[R["pos0_85"]]
    assert ((0, 0, 0) in hits.get(R["pos0_86"], [])) == later and ((0, 0, 0) in hits.get(R["pos0_120"], [])) == later
    # the first-window rule: a mismatch inside window 0 leaves the read to the later window, once
    if len(c.windows) > 1:
        base = {"": 0, "reads": 4, "db": 2}[c.x]  # an X against a base is a mismatch; X == X at 2 048 is none
        assert hits[R["long_0"]][0] == (0, lr.T0_AT, base)
        assert [h for h in hits[R["long_w0"]] if h[0] == 0] == [(0, lr.T0_AT, base + 1)]
    else:
        assert R["long_w0"] not in hits
    # two placements further apart than MMTol
    two = dict((g, nx) for g, p, nx in hits[R["long_0"]] if p == lr.T0_AT)
    assert set(two) == {0, 1} and abs(two[1] - two[0]) > lr.MMTOL
    best = set(map(tuple, lr.best_hits(name, lr.MMTOL).tolist()))
    assert (R["long_0"], 0, lr.T0_AT, two[0]) in best and (R["long_0"], 1, lr.T0_AT, two[1]) not in best
    assert len(best) < len(lr.oracle_hits(name))
    # nmiss beyond one byte, and the multiples of ten
    top = int(lr.oracle_hits(name)[:, 3].max())
    assert top == c.budget
    if c.lmax >= 4099:
        assert top > 255 and (top > 4095) == (c.lmax == 65535 and c.pmatch == 0.9)
    if c.pmatch == 0.9:
        assert c.ten == {1000: 1000, 4099: 4090, 65535: 65530}[c.lmax] and lr.budget(0.9, c.ten) == c.ten // 10 - 1
        assert (0, lr.T0_AT, c.ten // 10 - 1) in hits[R["ten_acc"]] and R["ten_rej"] not in hits
    else:
        assert c.ten == 0
    assert any(s[2] == 0.9 for s in lr.SPECS.values() if s[0] == c.lmax) or c.lmax == 1009
