"""Targets longer than 65 535 bases on every index kind, against oracle/literal.cpp.

Every index kind stores a placement's distances to its target's two ends in saturating 16-bit fields (context buckets:
kernels_match.hpp ctx_words / ctx_xtail / ctx_rem / ctx_fit, the last one saturating at 255 for a flagged entry;
window-start buckets: kernels_index.hpp k_index's lr word, screen_entry_ok, the descriptor's position field with its
pos_ok bit, k_confirm's pass 3, which recomputes a position from seq_off when pos_ok is clear), and exact code takes
over where a field saturates.  Every other module's targets have 1 000 bases or fewer (test_gpu_partitions.py has long
ones, compared with another GPU pass only), so none of that ran against the oracle before this module.

The database (seeded, 0.79 Mbase), in this order, so that neither the first nor the last target is ordinary and
seq_off[gene] != 0 for all long targets but one: 131 075 (contexts reach before the stream start), 300, 65 534, 0,
65 535, 8, 65 536, 65 537, 700, 70 001, 65 635, 196 613, 66 000 (contexts and gathers reach into the slack behind the
database).  A 150-base motif (250 for the runtime record stride) is planted nine times in six long targets: flush with
the end of two, at 65 535 - 20, at 0 of two, beyond 65 536, and in the middle of the 131 075- and 196 613-base ones
where both distances saturate; reads of the motif are the heavy (window, key) blocks MaxMatches needs.  The X database
is the same with about 0.1 % single X, four runs of 40 X (two of them beyond position 65 536 of a later target: three
and more X in one context, CTX_XMANY), single X 5-45 bases before the distances T - 256 .. T - 254 of three long
targets (flagged entries exactly where their distance saturates at 255) and 40 bases before the end of four (flagged
entries under the overhanging reads).

Reads: 64 * 16 + 37 distinct sorted reads per input, ragged as test_gpu_instances.make_reads makes them (lengths from
below the window width to the stride's longest, 30 % at full length, 1 % substitutions, the same X modes).  For every
window start q1 and every long target of T bases, each with a jitter of -1 / 0 / +1: p = 65 535 - q1 (left saturates),
p = T - 65 535 - q1 (right saturates), on the X database p = T - 255 - q1 (the flagged entry's saturation); reads
straddling and starting at 65 535 / 65 536, flush with the end, at p = 0 with lengths on both sides of 100 - ww and of
100 - (q1 + ww) (the literal 100 of the pos-0 rule, on targets whose saturated length is 65 535 + 65 535), uniform
positions in [65 536, T - L]; OVERHANGING reads (the target's last L - d bases and d = 1 or 5 random ones: the window
finds its key near the end, the fit rule must reject); 10 % from the motif, 10 % random.

test_inputs_are_hard (no GPU) asserts from the oracle's output alone that every input holds at least five accepted
tuples of every class named in CLASSES, at least 20 overhanging reads, hot probes at MaxMatches 25 and none at 10^6.
The GPU cases assert Engine.last_instance() first and then run test_gpu_instances.InstEngine.check (every tuple, best +
MMTol, MaxMatches 25, 1 and the sketch threshold, overflow_probes() a superset of the oracle's hot probes within
10 + len(hot) // 100) with MUSC_DEBUG_GRID=3.  MUSC_DEBUG_FORCE_WIDE=1 runs three two-kernel cases again on the entry
format of databases of 2^32 bases and more (24-bit target number, high offset byte in x); the download tests pack
positions of 18 bits and refuse 16; the partition tests cut the database at 60 000 bases, so that every long target
is a partition of its own and the motif's block spans partitions.

That the cases bite was checked with wrong forms of the arithmetic compiled in, one at a time: k_confirm's pass 3
ignoring pos_ok fails every two-kernel case (positions beyond 65 535 come back as 65 535 - q1); k_index storing
rem & 0xFFFF fails every two-kernel case; ctx_words doing the same fails every fused case; ctx_rem returning 16 bits of
a flagged entry fails the three fused cases on the X database; ctx_fit taking left == 0 from jx & 0xFFFF fails ten
fused cases.  A wide-format descriptor whose target number is not masked to 24 bits cannot fail on a database below
2^32 bases: bits 32-39 of every offset are zero there, so the mask is the identity (full-size runs cover it)."""
import ctypes
import os

import numpy as np
import pytest

from oracle import literal
from oracle import muscato_oracle as orc

from cases import hot_probes
from test_gpu_instances import GEOM, InstEngine, assert_same, oracle_full, with_mm

KNOBS = ("MUSC_INDEX", "MUSC_MATCH", "MUSC_NO_SPEC", "MUSC_DEBUG_CTX_DIRECT", "MUSC_DEBUG_INDEX_BITS", "MUSC_BATCH_READS",
         "MUSC_DEBUG_GRID", "MUSC_CONTEXT", "MUSC_DEBUG_FORCE_WIDE", "MUSC_SCREEN", "MUSC_NO_X_CONTEXT", "MUSC_GRAPH",
         "MUSC_PIPELINE")
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
X = ord("X")
N_READS = 64 * 16 + 37
SMALL_MM = 25
SAT = 65535

LENGTHS = (131075, 300, 65534, 0, 65535, 8, 65536, 65537, 700, 70001, 65635, 196613, 66000)
LONG = tuple(g for g, n in enumerate(LENGTHS) if n >= 65534)
# (target, position) of the motif's copies; -1: flush with the target's end
PLANTS = ((10, -1), (12, -1), (9, SAT - 20), (0, 0), (7, 0), (11, 150000), (0, 100000), (11, 98000), (0, 65536))
XRUNS = ((11, 120000), (9, 68000), (2, 30000), (0, 50000))  # runs of 40 X; the first two beyond 65 536 of a later target
XSAT_TARGETS = (9, 11, 12)
XSAT = ((256, 5), (255, 17), (254, 45))  # a single X b bases before the distance d to the target's end
XEND_TARGETS = (0, 7, 9, 11)             # a single X 40 bases before the end

SPEC = "spec"  # SpecGeom<1> (kernels_match_lane_inst.hpp): WindowWidth 15, Windows 0,20, MinDinuc 5
# input -> (geometry, windows, X mode, PMatch, MMTol, MatchMode, MinDinuc); a database with X gets PMatch <= 0.95 so that
# a read that overwrites three X of its target keeps a budget
INPUTS = {
    "8n-W1": ((8, False), 1, 0, 0.97, 0, "best", 0),
    "8n-W2": ((8, False), 2, 0, 0.95, 1, "first", 2),
    "8n-W3": ((8, False), 3, 0, 0.9, 3, "best", 4),
    "8n-W4": ((8, False), 4, 0, 0.97, 1, "first", 2),
    "8n-W2-x1": ((8, False), 2, 1, 0.9, 0, "best", 0),
    "8n-W2-x2": ((8, False), 2, 2, 0.9, 1, "best", 2),
    "8n-W3-x2": ((8, False), 3, 2, 0.95, 3, "first", 0),
    "12w-W2": ((12, True), 2, 0, 0.95, 0, "first", 4),
    "16w-W4": ((16, True), 4, 0, 0.9, 1, "best", 0),
    "12w-W2-x2": ((12, True), 2, 2, 0.9, 3, "first", 2),
    "spec": (SPEC, 2, 0, 0.97, 1, "best", 5),
    "rt-W3": ((0, False), 3, 0, 0.95, 1, "best", 2),
}
# class of accepted tuples -> what it reaches (test_inputs_are_hard: at least five of each per input)
CLASSES = {
    "far": "pos >= 65536 in a target whose number is > 0 (k_confirm's seq_off[gene] subtraction, positions wider than 16 bits)",
    "left_at": "pos + q1 == 65535 for some window: the first saturated left distance",
    "left_near": "pos + q1 in {65534, 65536}",
    "right_edge": "T - (pos + q1) in {65534, 65535, 65536}",
    "both": "both distances above 65535",
    "flush": "pos + len == T with T > 65535",
    "zero": "pos == 0 on a target whose saturated length is 65535 + 65535",
    "xsat": "XM = 2: the span holds an X of the target and T - (pos + q1) is in [201, 300] (a flagged entry's 255)",
    "xrun": "XM = 2: the span reaches into a run of 40 X beyond position 65536 of a later target (CTX_XMANY)",
}


def geometry(key):
    """-> (longest read, sorted window starts of all four windows, WindowWidth, motif length)"""
    if key == SPEC:
        return 100, (0, 20), 15, 150
    maxlen, wins, ww = GEOM[key]
    return maxlen, wins, ww, 250 if key == (0, False) else 150


# ---------------------------------------------------------------- inputs

_DB = {}


def database(mlen, with_x):
    """-> (targets, motif, literal.concat(targets), per target the sorted positions of its X)"""
    if (mlen, with_x) in _DB:
        return _DB[(mlen, with_x)]
    rng = np.random.default_rng(70 + mlen)
    T = [BASES[rng.integers(0, 4, size=n)] for n in LENGTHS]
    motif = BASES[rng.integers(0, 4, size=mlen)]
    if with_x:
        rx = np.random.default_rng(170 + mlen)
        for t in T:
            t[rx.random(len(t)) < 0.001] = X
    for g, p in PLANTS:
        p = LENGTHS[g] - mlen if p < 0 else p
        assert p + mlen <= LENGTHS[g]
        T[g][p:p + mlen] = motif
    if with_x:
        for g, p in XRUNS:
            T[g][p:p + 40] = X
        for g in XSAT_TARGETS:
            for d, b in XSAT:
                T[g][LENGTHS[g] - d - b] = X
        for g in XEND_TARGETS:
            T[g][LENGTHS[g] - 40] = X
    targets = [bytes(t) for t in T]
    xpos = [np.flatnonzero(t == X) for t in T]
    _DB[(mlen, with_x)] = (targets, bytes(motif), literal.concat(targets), xpos)
    return _DB[(mlen, with_x)]


def make_reads(seed, maxlen, wins, ww, xm, mlen):
    """-> (N_READS distinct sorted reads by the module docstring's recipe, the overhanging ones among them)"""
    targets, motif, _, _ = database(mlen, xm == 2)
    rng = np.random.default_rng(seed)
    inwin = np.zeros(maxlen, dtype=bool)
    for q in wins:
        inwin[q:q + ww] = True
    out, overhang, over = set(), set(), [0]

    def rlen(lo=None):
        lo = max(1, ww - 2) if lo is None else lo
        return maxlen if rng.random() < 0.3 else int(rng.integers(lo, maxlen + 1))

    def finish(r, sub=True):
        """substitutions and the X mode's treatment (test_gpu_instances.make_reads)"""
        L = len(r)
        isx = r == X
        if sub:
            s = (rng.random(L) < 0.01) & ~isx
            r[s] = BASES[rng.integers(0, 4, size=int(s.sum()))]
        if isx.any():  # XM = 2: random bases over the target's X, or keep up to three of them outside the windows
            keep = np.zeros(L, dtype=bool)
            if rng.random() < 0.5:
                keep = isx & ~inwin[:L]
                keep &= np.cumsum(keep) <= 3
            fill = isx & ~keep
            r[fill] = BASES[rng.integers(0, 4, size=int(fill.sum()))]
        if xm == 1:
            v = rng.random()
            if v < 0.25:
                r[rng.choice(L, size=min(L, int(rng.integers(1, 4))), replace=False)] = X
            elif v < 0.27 and 40 <= L <= 120 and over[0] < 12:  # more X than any budget, fewer than the count saturates at
                r[rng.choice(L, size=max(5, L // 10 + 2), replace=False)] = X
                over[0] += 1
        return bytes(r)

    def place(g, p, L, sub=True):
        if L >= 1 and p >= 0 and p + L <= LENGTHS[g]:
            out.add(finish(np.frombuffer(targets[g][p:p + L], dtype=np.uint8).copy(), sub))

    def through(g, p, q1, lo=None):
        """a read at p that is long enough for the window at q1, cut to the target's end"""
        L = min(rlen(q1 + ww if lo is None else lo), LENGTHS[g] - p)
        if L >= q1 + ww:
            place(g, p, L)

    out.add(bytes(BASES[rng.integers(0, 4, size=maxlen)]))  # (every window has a read long enough)
    for g in LONG:
        T = LENGTHS[g]
        for q1 in wins:
            for j in (-1, 0, 1):
                through(g, SAT - q1 + j, q1)
                through(g, T - SAT - q1 + j, q1)
                if xm == 2:
                    through(g, T - 255 - q1 + j, q1)
            for L in (100 - ww, 100 - ww + 1, 100 - (q1 + ww), 100 - (q1 + ww) + 1):
                if ww <= L <= maxlen:
                    place(g, 0, L)
        for _ in range(2):
            L = rlen()
            place(g, SAT + 1 - L, L)
            place(g, SAT, min(L, T - SAT))
            L = rlen()
            place(g, T - L, L)
        for d in (1, 5):
            for _ in range(2):
                L = rlen(wins[0] + ww + d)
                if L - d <= T:
                    r = np.concatenate([np.frombuffer(targets[g][T - (L - d):], dtype=np.uint8), BASES[rng.integers(0, 4, size=d)]])
                    r = finish(r, sub=False)
                    out.add(r)
                    overhang.add(r)
    if xm == 2:
        for g in XSAT_TARGETS:
            for _ in range(8):
                q1 = int(wins[rng.integers(0, len(wins))])
                through(g, LENGTHS[g] - q1 - int(rng.integers(201, 301)), q1)
        for g, s in XRUNS[:2]:
            for o in (1, 2, 3):
                for _ in range(2):
                    L = int(rng.integers(min(60, maxlen), maxlen + 1))
                    place(g, s + o - L, L)   # ends o bases into the run
                    place(g, s + 40 - o, L)  # starts o bases before its end
    nm = len(out) + N_READS // 10
    while len(out) < nm:  # the motif: seven in ten from its start (one heavy block per window), the others anywhere
        L = min(rlen(), mlen)
        o = 0 if rng.random() < 0.7 else int(rng.integers(0, mlen - L + 1))
        out.add(finish(np.frombuffer(motif[o:o + L], dtype=np.uint8).copy()))
    nr = len(out) + N_READS // 10
    while len(out) < nr:
        out.add(bytes(BASES[rng.integers(0, 4, size=rlen())]))
    assert len(out) < N_READS, len(out)
    far = [g for g in LONG if LENGTHS[g] - maxlen >= SAT + 1]
    while len(out) < N_READS:
        g = far[int(rng.integers(0, len(far)))]
        L = rlen()
        place(g, int(rng.integers(SAT + 1, LENGTHS[g] - L + 1)), L)
    assert xm != 1 or over[0] >= 3
    return sorted(out), overhang


def class_counts(full, reads, c, xpos):
    """Accepted tuples per class of CLASSES, from the oracle's tuples alone.  A window counts for a tuple when the read
    is long enough to have it."""
    r, g, p = (full[:, i].astype(np.int64) for i in range(3))
    L = np.array([len(x) for x in reads], dtype=np.int64)[r]
    T = np.array(LENGTHS, dtype=np.int64)[g]
    ww = c.WindowWidth
    z = np.zeros(len(full), dtype=bool)
    at, near, redge, both, xs = z.copy(), z.copy(), z.copy(), z.copy(), z.copy()
    for q1 in c.Windows:
        has = L >= q1 + ww
        jx = p + q1
        at |= has & (jx == SAT)
        near |= has & ((jx == SAT - 1) | (jx == SAT + 1))
        redge |= has & (np.abs(T - jx - SAT) <= 1)
        both |= has & (jx > SAT) & (T - jx > SAT)
        xs |= has & (T - jx >= 201) & (T - jx <= 300)
    nx = np.array([np.searchsorted(xpos[gi], pi + Li) - np.searchsorted(xpos[gi], pi) for gi, pi, Li in zip(g, p, L)], dtype=np.int64)
    run = z.copy()
    for rg, s in XRUNS[:2]:
        run |= (g == rg) & (p < s + 40) & (p + L > s)
    return {"far": int(((p >= SAT + 1) & (g > 0)).sum()), "left_at": int(at.sum()), "left_near": int(near.sum()),
            "right_edge": int(redge.sum()), "both": int(both.sum()), "flush": int(((p + L == T) & (T > SAT)).sum()),
            "zero": int(((p == 0) & (T > SAT)).sum()), "xsat": int((xs & (nx > 0)).sum()), "xrun": int(run.sum())}


_INPUT = {}


def build_input(name):
    """-> (config, reads, targets, every accepted tuple, hot probes at MaxMatches 25, overhanging reads, class counts),
    once per input: the oracle runs once for all the cases that share it."""
    if name in _INPUT:
        return _INPUT[name]
    key, W, xm, pmatch, mmtol, mode, mindinuc = INPUTS[name]
    maxlen, wins, ww, mlen = geometry(key)
    wins = sorted(wins[:W])
    c = orc.Config(Windows=wins, WindowWidth=ww, PMatch=pmatch, MinDinuc=mindinuc, MaxReadLength=maxlen, MaxMatches=1000000,
                   MMTol=mmtol, MatchMode=mode)
    targets, _, gcat, xpos = database(mlen, xm == 2)
    reads, overhang = make_reads(3000 + sorted(INPUTS).index(name), maxlen, wins, ww, xm, mlen)
    assert len(reads) == N_READS and max(map(len, reads)) == maxlen and min(map(len, reads)) < ww
    full = oracle_full(reads, c, gcat)
    hot = hot_probes(reads, targets, with_mm(c, SMALL_MM), full)
    _INPUT[name] = (c, reads, targets, full, hot, overhang, class_counts(full, reads, c, xpos))
    return _INPUT[name]


@pytest.mark.parametrize("name", list(INPUTS))
def test_inputs_are_hard(name):
    """The preconditions of the module docstring, from the oracle's output alone.  No GPU."""
    c, reads, targets, full, hot, overhang, counts = build_input(name)
    xm = INPUTS[name][2]
    print(name, len(full), counts, len(overhang), len(hot))
    for cls in CLASSES:
        if cls.startswith("x") and xm != 2:
            continue
        assert counts[cls] >= 5, "%s: %d accepted tuples of class %s (%s)" % (name, counts[cls], cls, CLASSES[cls])
    assert len(overhang) >= 20, (name, len(overhang))
    # an overhanging read has no placement where it was cut: the oracle ends every tuple inside its target
    L = np.array([len(r) for r in reads], dtype=np.int64)[full[:, 0]]
    assert (full[:, 2] + L <= np.array(LENGTHS, dtype=np.int64)[full[:, 1]]).all()
    assert hot, "%s: no block over MaxMatches %d" % (name, SMALL_MM)
    assert not hot_probes(reads, targets, c, full), "%s: a block over MaxMatches 10^6" % name


# ---------------------------------------------------------------- the case lists

def _t(rw, W, xm, wide, sg=0):
    return {"kernel": "k_match_t", "RW": rw, "W": W, "XM": xm, "WIDE": int(wide), "SG": sg}


def _scr(rw, mask, W, lines):
    return {"kernel": "k_screen", "RW": rw, "mask": mask, "one": int(W <= 2), "lines": lines}


def _conf(rw, mask, W):
    return {"kernel": "k_confirm", "RW": rw, "mask": mask, "w2": int(W <= 2)}


_SCR_T = {"kernel": "k_screen_t", "RW": 8}
CLASSIC, LINES = {"MUSC_INDEX": "classic"}, {"MUSC_INDEX": "lines"}
WIDE = {"MUSC_DEBUG_FORCE_WIDE": "1"}

# (id, {"match": ..} or {"screen": .., "confirm": ..}, knobs, input)
CASES = [("k_match_t<8,%d,0,false,0>" % W, {"match": _t(8, W, 0, False)}, {}, "8n-W%d" % W) for W in (1, 2, 3, 4)] + [
    ("k_match_t<8,2,1,false,0>", {"match": _t(8, 2, 1, False)}, {}, "8n-W2-x1"),
    ("k_match_t<8,2,2,false,0>", {"match": _t(8, 2, 2, False)}, {}, "8n-W2-x2"),
    ("k_match_t<8,3,2,false,0>", {"match": _t(8, 3, 2, False)}, {}, "8n-W3-x2"),
    ("k_match_t<12,2,0,true,0>", {"match": _t(12, 2, 0, True)}, {}, "12w-W2"),
    ("k_match_t<16,4,0,true,0>", {"match": _t(16, 4, 0, True)}, {}, "16w-W4"),
    ("k_match_t<12,2,2,true,0>", {"match": _t(12, 2, 2, True)}, {}, "12w-W2-x2"),
    ("k_match_g<8,0>", {"match": {"kernel": "k_match_g", "RW": 8, "SG": 0}}, {"MUSC_MATCH": "dma"}, "8n-W2"),
    # the direct 2^30-bucket table as test_gpu_spec.py reaches it; where it does not fit, the run falls back to another
    # index and the instance assertion fails
    ("k_match_t<8,2,0,false,1>", {"match": _t(8, 2, 0, False, 1)}, {"MUSC_DEBUG_CTX_DIRECT": "1"}, "spec"),
    ("k_match_g<8,1>", {"match": {"kernel": "k_match_g", "RW": 8, "SG": 1}}, {"MUSC_DEBUG_CTX_DIRECT": "1", "MUSC_MATCH": "dma"}, "spec"),
    # 2^14 buckets under a hash for 0.79 M window starts: every bucket holds colliding keys
    ("hashed-k_match_t<8,2,0,false,0>", {"match": _t(8, 2, 0, False)}, {"MUSC_DEBUG_INDEX_BITS": "14"}, "8n-W2"),
    ("classic-W2", {"screen": _scr(8, 0, 2, 0), "confirm": _conf(8, 0, 2)}, CLASSIC, "8n-W2"),
    ("classic-W3", {"screen": _scr(8, 0, 3, 0), "confirm": _conf(8, 0, 3)}, CLASSIC, "8n-W3"),
    ("classic-W2-mask-reads", {"screen": _scr(8, 1, 2, 0), "confirm": _conf(8, 1, 2)}, CLASSIC, "8n-W2-x1"),
    ("classic-W3-mask-database", {"screen": _scr(8, 1, 3, 0), "confirm": _conf(8, 1, 3)}, CLASSIC, "8n-W3-x2"),
    ("classic-runtime-stride-W3", {"screen": _scr(0, 0, 3, 0), "confirm": _conf(0, 0, 3)}, CLASSIC, "rt-W3"),
    ("lines-k_screen_t<8>-W2", {"screen": _SCR_T, "confirm": _conf(8, 0, 2)}, LINES, "8n-W2"),
    ("lines-k_screen_t<8>-W3", {"screen": _SCR_T, "confirm": _conf(8, 0, 3)}, LINES, "8n-W3"),
    ("lines-wg-k_screen<8,0,1,1>", {"screen": _scr(8, 0, 2, 1), "confirm": _conf(8, 0, 2)}, dict(LINES, MUSC_SCREEN="wg"), "8n-W2"),
    ("lines-W3-mask-database", {"screen": _scr(8, 1, 3, 1), "confirm": _conf(8, 1, 3)}, LINES, "8n-W3-x2"),
    ("wide-classic-W2", {"screen": _scr(8, 0, 2, 0), "confirm": _conf(8, 0, 2)}, dict(CLASSIC, **WIDE), "8n-W2"),
    ("wide-lines-k_screen_t<8>-W3", {"screen": _SCR_T, "confirm": _conf(8, 0, 3)}, dict(LINES, **WIDE), "8n-W3"),
    ("wide-classic-W3-mask-database", {"screen": _scr(8, 1, 3, 0), "confirm": _conf(8, 1, 3)}, dict(CLASSIC, **WIDE), "8n-W3-x2"),
]


def test_case_list():
    """Every case names an input, ids are distinct, every input has a case.  No GPU."""
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids)) == 26
    assert {c[3] for c in CASES} == set(INPUTS)
    for key, W, _, _, _, _, _ in INPUTS.values():
        maxlen, wins, ww, mlen = geometry(key)
        assert max(wins[:W]) + ww <= maxlen <= 250 and mlen <= min(LENGTHS[g] for g, _ in PLANTS)


# ---------------------------------------------------------------- the GPU side

@pytest.fixture(scope="module")
def ie():
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    s = InstEngine()
    try:
        yield s
    finally:
        s.e.close()
        for k in KNOBS:
            os.environ.pop(k, None)
        for k, v in old.items():
            if v is not None:
                os.environ[k] = v


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_long_targets(ie, i):
    name, want, knobs, inp = CASES[i]
    c, reads, targets, full, hot, _, _ = build_input(inp)
    ie.check(name, want, knobs, c, reads, targets, full, hot)  # (asserts last_instance() before any tuple)
    if "MUSC_DEBUG_FORCE_WIDE" in knobs:
        # the knob bars context buckets: 64-byte buckets (0) or line buckets (3), in the wide entry format
        assert ie.e.stats()["index_kind"] == (3 if knobs["MUSC_INDEX"] == "lines" else 0), name


def _first_pass(ie, want, knobs, inp):
    """Every accepted tuple of an input on the device, instance asserted first; -> (engine, tuples, reads)"""
    c, reads, targets, full, _, _, _ = build_input(inp)
    ie.set_knobs(knobs)
    ie.load(targets, reads)
    got, _, li = ie.run(c, False)
    for k in ("match", "screen", "confirm"):
        assert li[k] == want.get(k), (li, want)
    assert_same(got, full, "downloads " + inp)
    assert int(full[:, 2].max()) >= SAT + 1
    return ie.e, full, reads


_HIP = []


def _hip():
    if not _HIP:
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        hip.hipFree.argtypes = [ctypes.c_void_p]
        _HIP.append(hip)
    return _HIP[0]


DOWNLOADS = [("fused", {"match": _t(8, 2, 0, False)}, {}), ("two-kernel", {"screen": _scr(8, 0, 2, 0), "confirm": _conf(8, 0, 2)}, CLASSIC)]


@pytest.mark.gpu
@pytest.mark.parametrize("path", range(2), ids=[d[0] for d in DOWNLOADS])
def test_downloads_with_wide_positions(ie, path):
    """musc_hits_copy_packed with 18 position bits and musc_hits_copy_compact with gene 4 / pos 18 / nmiss 8, to host and
    to device memory, round-trip to exactly the musc_hit tuples (which equal the oracle's); 16 position bits are refused."""
    from muscato_amd import sorted_hits
    _, want, knobs = DOWNLOADS[path]
    e, full, reads = _first_pass(ie, want, knobs, "8n-W2")
    n, nr = len(full), len(reads)
    hip = _hip()
    bits = [11, 4, 18, 8]
    words = np.zeros(n, dtype=np.uint64)
    e.hits_to_packed(words.ctypes.data, n, False, bits, 0)
    back = np.zeros((n, 4), dtype=np.uint32)
    e.unpack_hits(words.ctypes.data, n, False, bits, back.ctypes.data)
    assert_same(sorted_hits(back), full, "packed, host")
    assert (((words >> np.uint64(8)) & np.uint64((1 << 18) - 1)) == back[:, 2]).all()
    cbits = [4, 18, 8]
    cw = np.zeros(n, dtype=np.uint32)
    cc = np.full(nr, 77, dtype=np.uint8)
    e.hits_to_compact(cw.ctypes.data, n, cc.ctypes.data, nr, False, cbits)
    assert (cc == np.bincount(full[:, 0], minlength=nr)).all()
    rd = np.repeat(np.arange(nr, dtype=np.uint32), cc)
    dec = np.stack([rd, cw >> 26, (cw >> 8) & 0x3FFFF, cw & 0xFF], axis=1).astype(np.uint32)
    assert_same(sorted_hits(dec), full, "compact, host")
    dw, dh, dc = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dw), n * 8 + 16) == 0 and hip.hipMalloc(ctypes.byref(dh), n * 16) == 0
    assert hip.hipMalloc(ctypes.byref(dc), nr + 16) == 0
    try:
        e.hits_to_packed(dw.value, n, True, bits, 0)
        w2 = np.zeros(n, dtype=np.uint64)
        assert hip.hipMemcpy(w2.ctypes.data, dw, n * 8, 2) == 0
        assert (w2 == words).all()
        e.unpack_hits(dw.value, n, True, bits, dh.value)
        h2 = np.zeros((n, 4), dtype=np.uint32)
        assert hip.hipMemcpy(h2.ctypes.data, dh, n * 16, 2) == 0
        assert_same(sorted_hits(h2), full, "packed, device")
        e.hits_to_compact(dw.value, n, dc.value, nr, True, cbits)
        cw2, cc2 = np.zeros(n, dtype=np.uint32), np.zeros(nr, dtype=np.uint8)
        assert hip.hipMemcpy(cw2.ctypes.data, dw, n * 4, 2) == 0 and hip.hipMemcpy(cc2.ctypes.data, dc, nr, 2) == 0
        assert (cw2 == cw).all() and (cc2 == cc).all()
        for on_device, pw, pc in ((False, words.ctypes.data, cc.ctypes.data), (True, dw.value, dc.value)):
            with pytest.raises(RuntimeError, match="does not fit"):
                e.hits_to_packed(pw, n, on_device, [11, 4, 16, 8], 0)
            with pytest.raises(RuntimeError, match="does not fit"):
                e.hits_to_compact(pw, n, pc, nr, on_device, [4, 16, 8])
    finally:
        hip.hipFree(dw)
        hip.hipFree(dh)
        hip.hipFree(dc)


def greedy_plan(limit):
    """include/muscato_hip.h, musc_db_set_partition_bases: ranges of whole targets of at most `limit` bases, taken
    greedily from the first target on; a longer target is a range of its own."""
    plan, g = [0], 0
    while g < len(LENGTHS):
        g1, s = g, 0
        while g1 < len(LENGTHS) and s + LENGTHS[g1] <= limit:
            s += LENGTHS[g1]
            g1 += 1
        g = max(g1, g + 1)
        plan.append(g)
    return plan


def test_greedy_plan_model():
    """At 60 000 bases every long target is alone; the targets of this database alternate, so no two short ones are
    neighbours and every range holds one target (the empty one included).  A limit that admits two targets joins them.
    No GPU."""
    assert greedy_plan(60000) == list(range(len(LENGTHS) + 1))
    assert greedy_plan(66000) == [0, 1, 4, 6, 7, 8, 9, 10, 11, 12, 13]  # 300 + 65534 + 0 and 65535 + 8 fit 66000


PARTITIONED = [("context", {"match": _t(8, 2, 0, False)}, {}, "8n-W2"), ("lines", {"screen": _SCR_T, "confirm": _conf(8, 0, 3)}, LINES, "8n-W3")]


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [60000, 66000])
@pytest.mark.parametrize("path", range(2), ids=[p[0] for p in PARTITIONED])
def test_partitions_of_long_targets(ie, path, limit):
    """musc_db_set_partition_bases(60000): every long target is a partition of its own (66000: the short ones share one
    with a neighbour where the limit allows), the motif's block spans partitions, and every tuple, best + MMTol and the
    MaxMatches-25 verdict and probes equal the unpartitioned pass's and the oracle's."""
    _, want, knobs, inp = PARTITIONED[path]
    c, reads, targets, full, hot, _, _ = build_input(inp)
    best = np.array(sorted(orc.best_filter(map(tuple, full.tolist()), c.MMTol)), dtype=np.uint32).reshape(-1, 4)
    assert len({g for g, _ in PLANTS}) >= 6  # (the motif's copies lie in six targets: in six partitions)
    ie.set_knobs(knobs)
    ie.load(targets, reads)
    seen = {}
    try:
        for lim in (0, limit):
            ie.e.set_partition_bases(lim)
            what = "%s, partition limit %d" % (inp, lim)
            got, st, li = ie.run(c, False)
            for k in ("match", "screen", "confirm"):
                assert li[k] == want.get(k), (what, li)
            plan = ie.e.partitions()
            assert plan == (greedy_plan(lim) if lim else [0, len(LENGTHS)]), (what, plan)
            for g in LONG if lim == 60000 else ():
                assert g in plan and g + 1 in plan, (what, g, plan)
            assert_same(got, full, what)
            assert st["n_hits"] == len(full) and st["n_overflow_blocks"] == 0, (what, st)
            got, st, _ = ie.run(c, True)
            assert_same(got, best, what + " best+MMTol")
            got, st, _ = ie.run(with_mm(c, SMALL_MM), False)
            assert_same(got, full, what + " MaxMatches 25")
            probes = set(map(tuple, ie.e.overflow_probes().tolist()))
            assert st["n_overflow_blocks"] >= 1 and hot <= probes and len(probes - hot) <= 10 + len(hot) // 100, \
                (what, st["n_overflow_blocks"], len(hot), len(hot - probes), len(probes - hot))
            seen[lim] = probes
        assert seen[limit] >= seen[0]
    finally:
        ie.e.set_partition_bases(0)
