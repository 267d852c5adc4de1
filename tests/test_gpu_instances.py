"""Every compiled kernel instance of the hot path against the CPU oracle, one parametrised case per instance.

The host picks one instance per pass out of about 150: k_match_t<RW, W, XM, WIDE, SG> (84 general ones: record stride
4 / 8 / 12 words on 120-base buckets and 4 / 8 / 12 / 16 on wide ones, 1-4 windows, three X modes -- and the template
arguments switch real code: the candidate list shrinks from 96 to 64 entries for RW >= 12, BB_LDS exists only for
W == 3 && XM == 0 && RW <= 8, OWNK only for W <= 2 && XM == 0 && !WIDE, W == 1 has its own schedule), k_match_g<8, 0>,
and on the two-kernel path k_screen<RW, mask, one, lines> (40), k_screen_t<RW> (4) and k_confirm<RW, mask, w2> (20).
Engine.last_instance() reports, from the resolver that returned the function pointer, which of them a pass launched;
every case here asserts it FIRST, so a silent fall-back to another instance fails instead of passing, and then compares
with oracle/literal.cpp (never with another GPU path):

  - every accepted tuple (apply_mmtol=False, MaxMatches 10^6) and the stats invariants;
  - best + MMTol, with PMatch, MMTol, MatchMode and MinDinuc varied pairwise over the cases;
  - MaxMatches 1 (every probe of a block of two or more accepted pairs named: the threshold where most blocks are),
    MaxMatches 25 (exact block counters at once) and the smallest MaxMatches that starts with the screening sketch,
    which a read of the motif trips into the exact re-run (asserted: last_instance()["exact_rerun"]): tuples unchanged,
    n_overflow_blocks >= 1 exactly when an oracle block overflows, overflow_probes() a superset of the oracle's hot
    probes with at most 10 + len(hot) // 100 extra (the margin of test_gpu_spec.py).

Inputs (seeded): a database of 300 targets of 700 bases, a quarter of them mutated copies, a 200-base motif planted in
40 of them (heavy blocks) and 24 targets shorter than a read, one per X mode; 64 * 40 + 37 distinct reads per case
(a ragged last wave-tile; 64 * 16 + 37 on the two-kernel path), lengths from below the window width to the stride's
longest, 30 % at full length, placements at position 0 and flush with the target end, 10 % from the motif, 12 % random,
1 % substitutions.  MUSC_DEBUG_GRID=3: one wave walks many wave-tiles.  Each case asserts from the ORACLE's output
that it is hard: some tile of 64 reads accepts more than 96 tuples (k_match_t's candidate list spills in both its
sizes), hot probes at MaxMatches 25 and none at 10^6.

X modes: XM = 0 no X; XM = 1 X in the reads only, at most three per read (every read lists them in its xpos word at
any PMatch) plus a few reads with more X than any mismatch budget; XM = 2 a database with X at about 0.1 % (single
bases and runs of 40), half of the reads sampled over an X get random bases there, the others keep the target's X, three
at most and only outside their windows (a read with X inside a window against a database with X leaves the context
path, and the instance assertion would fail).

Instances only a knob reaches.  A run that chooses its own bucket width cannot reach k_match_t<4, 1, *, true> and
<8, 1, *, true> (one window goes wide only with reads over 120 bases: stride 12), and reaches <4, 2..4, *, true> only
with a last window no read is long enough for (`Windows 0,100`, 40-base reads: kept here as a case of its own).  Those
fifteen run with MUSC_CONTEXT=wide, which puts every run on wide buckets.  k_screen<RW != 0, false, *, true> (line
buckets, no mask plane) runs only with MUSC_SCREEN=wg: without it such a run takes k_screen_t<RW>.  No instance of the
resolvers' tables is unreachable; test_every_instance_has_a_case (no GPU) compares the case lists with
musc_instances(), the resolvers' own enumeration, and with MUSC_LANE_INSTANCES_* of kernels_match_lane_inst.hpp, so an
instance added without a case fails the suite.  The geometry-specialised k_match_t<8, 2, 0, false, 1> and k_match_g<8, 1>
are test_gpu_spec.py's."""
import os
import re

import numpy as np
import pytest

from oracle import literal
from oracle import muscato_oracle as orc

from cases import hot_probes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("MUSC_INDEX", "MUSC_MATCH", "MUSC_NO_SPEC", "MUSC_DEBUG_CTX_DIRECT", "MUSC_DEBUG_INDEX_BITS", "MUSC_BATCH_READS",
         "MUSC_DEBUG_GRID", "MUSC_CONTEXT", "MUSC_DEBUG_FORCE_WIDE", "MUSC_SCREEN", "MUSC_NO_X_CONTEXT", "MUSC_GRAPH",
         "MUSC_PIPELINE")
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
X = ord("X")
N_FUSED = 64 * 40 + 37
N_TWO = 64 * 16 + 37
MAX_GRID = 4096  # kernels_common.hpp: the host's screening threshold is MaxMatches / (planned batches * MAX_GRID)
SMALL_MM = 25
WLIST = 96       # k_match_t's larger candidate list (MATCHT_WLIST; 64 for RW >= 12)

# (RW, wide buckets) -> longest read, window starts (a case takes the first W, sorted), WindowWidth.
# rw = roundup4(ceil(2 * maxlen / 32) + 1); max(win) - min(win) + maxlen over 120 is wide, over 200 leaves the context
# path; every window is reachable by a full-length read.
GEOM = {
    (4, False): (48, (0, 9, 18, 27), 8),
    (8, False): (100, (0, 20, 7, 13), 12),
    (12, False): (114, (0, 6, 2, 4), 10),
    (8, True): (104, (3, 90, 40, 65), 11),
    (12, True): (150, (0, 50, 20, 35), 15),
    (16, True): (178, (0, 22, 8, 15), 13),
    (0, False): (250, (0, 60, 130, 200), 12),  # the runtime stride (20 words): the two-kernel path only
}
PMATCH = (0.97, 0.95, 0.9)
MMTOL = (0, 1, 3)
MINDINUC = (0, 2, 4)


def record_stride(maxlen):
    return (-(-2 * maxlen // 32) + 1 + 3) // 4 * 4


def _params(i, wins, ww, maxlen):
    """Run parameters of case number i: PMatch x MMTol x MatchMode x MinDinuc, pairwise over the cases."""
    return orc.Config(Windows=sorted(wins), WindowWidth=ww, PMatch=PMATCH[i % 3], MinDinuc=MINDINUC[(i // 3 + i) % 3],
                      MaxReadLength=maxlen, MaxMatches=1000000, MMTol=MMTOL[(i // 3) % 3], MatchMode=("best", "first")[(i + i // 9) % 2])


# ---------------------------------------------------------------- the case lists (no GPU)

def fused_cases():
    """-> [(id, descriptor, knobs, geometry key, W, xm)], one per general k_match_t instance and k_match_g<8, 0>, and
    the natural dead-window case."""
    out = []
    for xm in (0, 1, 2):
        for (rw, wide) in ((4, False), (8, False), (12, False), (4, True), (8, True), (12, True), (16, True)):
            for W in (1, 2, 3, 4):
                knobs, key = {}, (rw, wide)
                if wide and (rw == 4 or (rw == 8 and W == 1)):
                    knobs, key = {"MUSC_CONTEXT": "wide"}, (rw, False)  # (the docstring: only the knob reaches them)
                d = {"kernel": "k_match_t", "RW": rw, "W": W, "XM": xm, "WIDE": int(wide), "SG": 0}
                out.append(("k_match_t<%d,%d,%d,%s,0>" % (rw, W, xm, "true" if wide else "false"), d, knobs, key, W, xm))
    out.append(("k_match_g<8,0>", {"kernel": "k_match_g", "RW": 8, "SG": 0}, {"MUSC_MATCH": "dma"}, (8, False), 2, 0))
    out.append(("k_match_t<4,2,0,true,0>-dead-window", {"kernel": "k_match_t", "RW": 4, "W": 2, "XM": 0, "WIDE": 1, "SG": 0},
                {}, "dead", 2, 0))
    return out


def two_kernel_cases():
    """-> [(id, screen descriptor, confirm descriptor, knobs, geometry key, W, xm)]: MUSC_INDEX=classic and =lines, every
    record stride with instances of its own and the runtime one, with and without the mask plane (X in the reads for two
    windows, in the database for three), W <= 2 and W > 2; on line buckets without a mask plane k_screen_t<RW> and,
    with MUSC_SCREEN=wg, k_screen<RW, false, *, true>."""
    out = []
    for index in ("classic", "lines"):
        lines = int(index == "lines")
        for rw in (4, 8, 12, 16, 0):
            for mask in (0, 1):
                for W in (2, 3):
                    one = int(W <= 2)
                    key = (rw, rw == 16)
                    xm = 0 if not mask else 1 if W == 2 else 2
                    conf = {"kernel": "k_confirm", "RW": rw, "mask": mask, "w2": one}
                    scr = {"kernel": "k_screen", "RW": rw, "mask": mask, "one": one, "lines": lines}
                    knobs = {"MUSC_INDEX": index}
                    if lines and not mask and rw:
                        out.append(("%s-k_screen_t<%d>-W%d+k_confirm<%d,false,%d>" % (index, rw, W, rw, one),
                                    {"kernel": "k_screen_t", "RW": rw}, conf, dict(knobs), key, W, xm))
                        knobs["MUSC_SCREEN"] = "wg"
                    out.append(("%s-k_screen<%d,%d,%d,%d>+k_confirm<%d,%d,%d>" % (index, rw, mask, one, lines, rw, mask, one),
                                scr, conf, knobs, key, W, xm))
    return out


FUSED = fused_cases()
TWO = two_kernel_cases()


def _key(d):
    return tuple(sorted(d.items()))


def test_every_instance_has_a_case():
    """The case lists against the library's own enumeration of its resolvers (musc_instances: every descriptor
    match_instance / screen_instance / screen_t_instance / confirm_instance can return) and against the
    instantiation lists of kernels_match_lane_inst.hpp.  No GPU."""
    from muscato_amd.api import instances
    have = {}
    for d in instances():
        have.setdefault(d["kernel"], set()).add(_key(d))
    assert {k: len(v) for k, v in have.items()} == {"k_match_t": 85, "k_match_g": 2, "k_screen": 40, "k_screen_t": 4, "k_confirm": 20}
    spec = {_key({"kernel": "k_match_t", "RW": 8, "W": 2, "XM": 0, "WIDE": 0, "SG": 1}), _key({"kernel": "k_match_g", "RW": 8, "SG": 1})}
    ids = [c[0] for c in FUSED] + [c[0] for c in TWO]
    assert len(ids) == len(set(ids))
    fused = {_key(c[1]) for c in FUSED}
    assert len(FUSED) == 84 + 1 + 1 and len(fused) == 84 + 1
    assert fused == (have["k_match_t"] | have["k_match_g"]) - spec  # (test_gpu_spec.py runs the specialised two)
    assert {_key(c[1]) for c in TWO} == have["k_screen"] | have["k_screen_t"]
    assert {_key(c[2]) for c in TWO} == have["k_confirm"]
    # the translation units instantiate exactly what the resolvers' tables name
    with open(os.path.join(ROOT, "muscato_amd", "csrc", "kernels_match_lane_inst.hpp")) as f:
        hdr = f.read()
    per_wd = re.findall(r"k_match_t<RW, (\d), (\d), WD, 0>", hdr.split("#define MUSC_LANE_INSTANCES_WD")[1].split("// 120-base")[0])
    rows = re.findall(r"#define MUSC_LANE_INSTANCES_\w+\(X\)((?: MUSC_LANE_INSTANCES_WD\(X, \d+, \w+\))+)", hdr)
    wd = [(int(rw), w == "true") for row in rows for rw, w in re.findall(r"WD\(X, (\d+), (\w+)\)", row)]
    compiled = {_key({"kernel": "k_match_t", "RW": rw, "W": int(W), "XM": int(xm), "WIDE": int(wide), "SG": 0})
                for rw, wide in wd for W, xm in per_wd}
    assert len(per_wd) == 12 and len(wd) == 7 and len(compiled) == 84
    assert compiled == {k for k in have["k_match_t"] if dict(k)["SG"] == 0}
    assert re.findall(r"k_match_g<(\d+), (\d)> MUSC_MATCH_ARGS;", hdr) == [("8", "0"), ("8", "1")]
    # every geometry gives the record stride and the bucket width its case names
    for (rw, wide), (maxlen, wins, ww) in GEOM.items():
        assert record_stride(maxlen) == (rw or 20)
        for W in (1, 2, 3, 4):
            w = sorted(wins[:W])
            span = w[-1] - w[0] + maxlen
            assert w[-1] + ww <= maxlen
            if rw:
                assert (span > 120) == wide or (wide and W == 1 and rw == 8), (rw, wide, W)
                assert span <= 200


# ---------------------------------------------------------------- inputs

_DB = {}


def database(xm):
    """(targets, motif) of an X mode: XM 0 and 1 share the X-free one."""
    with_x = xm == 2
    if with_x in _DB:
        return _DB[with_x]
    rng = np.random.default_rng(40 + with_x)
    n, tlen = 300, 700
    T = BASES[rng.integers(0, 4, size=(n, tlen))]
    ncopy = n // 4
    T[n - ncopy:] = T[rng.integers(0, n - ncopy, size=ncopy)]
    sub = rng.random((ncopy, tlen)) < 0.03
    T[n - ncopy:][sub] = BASES[rng.integers(0, 4, size=int(sub.sum()))]
    motif = BASES[rng.integers(0, 4, size=200)]
    for i in rng.choice(n - ncopy, size=40, replace=False):
        p = int(rng.integers(0, tlen - 200 + 1))
        T[i, p:p + 200] = motif
    if with_x:
        T[rng.random(T.shape) < 0.001] = X
        for i in rng.choice(n, size=4, replace=False):
            p = int(rng.integers(0, tlen - 40 + 1))
            T[i, p:p + 40] = X
    targets = [bytes(t) for t in T]
    for i in range(24):  # shorter than the long reads, some than every read
        m = int(rng.integers(12, 170))
        targets.append(bytes(motif[:m]) if i % 3 == 0 else bytes(BASES[rng.integers(0, 4, size=m)]))
    _DB[with_x] = (targets, bytes(motif), literal.concat(targets))
    return _DB[with_x]


def make_reads(seed, n, maxlen, wins, ww, xm):
    """n distinct sorted reads by the module docstring's recipe."""
    targets, motif, _ = database(xm)
    rng = np.random.default_rng(seed)
    tl = np.array([len(t) for t in targets])
    inwin = np.zeros(maxlen, dtype=bool)
    for q in wins:
        inwin[q:q + ww] = True
    out = {bytes(BASES[rng.integers(0, 4, size=maxlen)])}  # (every window has a read long enough)
    over = 0
    while len(out) < n:
        L = maxlen if rng.random() < 0.3 else int(rng.integers(max(1, ww - 2), maxlen + 1))
        u = rng.random()
        if u < 0.12:
            r = BASES[rng.integers(0, 4, size=L)]
        else:
            if u < 0.22 and L <= len(motif):
                o = int(rng.integers(0, len(motif) - L + 1))
                r = np.frombuffer(motif[o:o + L], dtype=np.uint8).copy()
            else:
                fit = np.flatnonzero(tl >= L)
                g = int(fit[rng.integers(0, len(fit))])
                v = rng.random()
                p = 0 if v < 0.05 else int(tl[g]) - L if v < 0.1 else int(rng.integers(0, tl[g] - L + 1))
                r = np.frombuffer(targets[g][p:p + L], dtype=np.uint8).copy()
            isx = r == X
            sub = (rng.random(L) < 0.01) & ~isx
            r[sub] = BASES[rng.integers(0, 4, size=int(sub.sum()))]
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
                r = r.copy()
                r[rng.choice(L, size=min(L, int(rng.integers(1, 4))), replace=False)] = X
            elif v < 0.27 and 40 <= L <= 120 and over < 12:
                # more X than the xpos word lists (four; three on wide buckets) and than the budget int((1 - PMatch) * L)
                # at PMatch >= 0.9 -- and fewer than 15, where the word's count saturates and the run would leave the
                # context path
                r = r.copy()
                r[rng.choice(L, size=max(5, L // 10 + 2), replace=False)] = X
                over += 1
        out.add(bytes(r))
    assert xm != 1 or over >= 3
    return sorted(out)


def oracle_full(reads, c, gcat):
    gbuf, goff = gcat
    rbuf, roff = literal.concat(reads)
    big = orc.Config(**dict(c.__dict__, MaxMatches=2 ** 31 - 1))
    exp, _, _ = literal.match_arrays(rbuf, roff, gbuf, goff, literal.make_params(big, bloom_size=16_000_000, num_hash=6, nthreads=8))
    return exp


def with_mm(c, mm):
    return orc.Config(**dict(c.__dict__, MaxMatches=mm))


def build_case(i, key, W, xm, n):
    """-> (config, reads, targets, every accepted tuple, hot probes at MaxMatches 25), preconditions asserted."""
    if key == "dead":
        maxlen, wins, ww = 40, (0, 100), 12
    else:
        maxlen, wins, ww = GEOM[key]
        wins = wins[:W]
    c = _params(i, wins, ww, maxlen)
    targets, _, gcat = database(xm)
    reads = make_reads(1000 + i, n, maxlen, c.Windows, ww, xm)
    assert len(reads) == n and n % 64 == 37 and max(map(len, reads)) == maxlen and min(map(len, reads)) < ww
    # (the dead-window case: oracle/literal refuses a window no read is long enough for, as the reference exits
    # there; such a window has no probe, so the accepted tuples are those of the live windows alone)
    live = [q for q in c.Windows if q + ww <= maxlen]
    full = oracle_full(reads, orc.Config(**dict(c.__dict__, Windows=live)), gcat)
    per_tile = np.bincount(full[:, 0] // 64, minlength=(n + 63) // 64)
    assert per_tile.max() > WLIST, "no tile of 64 reads accepts more than %d tuples (most: %d)" % (WLIST, per_tile.max())
    hot = hot_probes(reads, targets, with_mm(c, SMALL_MM), full)
    assert hot, "no block over MaxMatches %d" % SMALL_MM
    assert not hot_probes(reads, targets, c, full), "a block over MaxMatches 10^6"
    return c, reads, targets, full, hot


def to_cfg(c):
    from muscato_amd import Config
    return Config(Windows=list(c.Windows), WindowWidth=c.WindowWidth, PMatch=c.PMatch, MinDinuc=c.MinDinuc,
                  MaxReadLength=c.MaxReadLength, MaxMatches=c.MaxMatches, MMTol=c.MMTol, MatchMode=c.MatchMode)


def assert_same(got, exp, what):
    """Every tuple: the first difference names its read, target, position."""
    if got.shape == exp.shape and (got == exp).all():
        return
    g, e = set(map(tuple, got.tolist())), set(map(tuple, exp.tolist()))
    assert False, "%s: gpu %d tuples, oracle %d; missing %s, extra %s" % (what, len(got), len(exp), sorted(e - g)[:5], sorted(g - e)[:5])


# ---------------------------------------------------------------- the GPU side

class InstEngine:
    """One Engine for the module (modelled on test_gpu_spec.py's SpecEngine): the database and knobs it holds."""

    def __init__(self):
        from muscato_amd import Engine
        self.e = Engine(0)
        self.targets = None
        self.knobs = {}

    def set_knobs(self, knobs):
        knobs = dict(knobs, MUSC_DEBUG_GRID=knobs.get("MUSC_DEBUG_GRID", "3"))
        if knobs == self.knobs:
            return
        for k in KNOBS:
            os.environ.pop(k, None)
        for k, v in knobs.items():
            if v is not None:
                os.environ[k] = v
        self.knobs = knobs
        self.e.reload_env()

    def load(self, targets, reads):
        if self.targets is not targets:
            self.e.load_targets(targets)
            self.targets = targets
        self.e.load_reads(reads)

    def run(self, c, apply_mmtol):
        from muscato_amd import sorted_hits
        got = sorted_hits(self.e.match(to_cfg(c), apply_mmtol=apply_mmtol))
        return got, self.e.stats(), self.e.last_instance()

    def check(self, what, want, knobs, c, reads, targets, full, hot):
        """The checks of the module docstring.  want: {"match": descriptor} or {"screen": .., "confirm": ..}."""
        n = len(reads)
        self.set_knobs(knobs)
        self.load(targets, reads)

        def same_instance(li, w):
            for k in ("match", "screen", "confirm"):
                assert li[k] == want.get(k), "%s %s: launched %s, the case is written for %s" % (what, w, li[k], want.get(k))

        # every accepted tuple, MaxMatches 10^6: no block check can be inconclusive there, no overflow
        got, st, li = self.run(c, False)
        same_instance(li, "all tuples")
        assert_same(got, full, what + " all tuples")
        assert st["n_reads"] == n and st["n_pairs"] >= st["n_accepted"] >= st["n_hits"] == len(full), (what, st)
        assert st["n_overflow_blocks"] == 0, (what, st["n_overflow_blocks"])
        # best + MMTol
        best, st, li = self.run(c, True)
        same_instance(li, "best+MMTol")
        exp = np.array(sorted(orc.best_filter(map(tuple, full.tolist()), c.MMTol)), dtype=np.uint32).reshape(-1, 4)
        assert_same(best, exp, what + " best+MMTol")
        assert st["n_reads"] == n and st["n_pairs"] >= st["n_accepted"] >= st["n_hits"] == len(exp), (what, st)
        # MaxMatches 25: exact block counters at once
        c25 = with_mm(c, SMALL_MM)
        got, st, li = self.run(c25, False)
        same_instance(li, "MaxMatches 25")
        assert li["block_mode"] == 2 and not li["exact_rerun"], (what, li)
        assert_same(got, full, what + " MaxMatches 25")
        assert st["n_overflow_blocks"] >= 1, what
        probes = set(map(tuple, self.e.overflow_probes().tolist()))
        assert hot <= probes and len(probes - hot) <= 10 + len(hot) // 100, (what, len(hot), len(hot - probes), len(probes - hot))
        # MaxMatches 1: the threshold where most blocks are.  A block of this data holds 1-4 accepted pairs (a target and
        # its mutated copies) or 40 and more (the motif), so at 25 a count that is off by a few flips no verdict; at 1 a
        # block of two pairs that loses one is no longer named.  Only the side that must hold is asserted: every probe of
        # an overflowing block is named.  The bound on extra probes is not applied here: the counters are 2^22 hashed
        # cells, at this threshold any two blocks that share a cell are both named, and their number grows with the
        # square of the block count (measured: up to 42 extra on 2 667 hot probes).
        cm = with_mm(c, 1)
        hotm = hot_probes(reads, targets, cm, full)
        assert len(hotm) > len(hot), what
        got, st, li = self.run(cm, False)
        same_instance(li, "MaxMatches 1")
        assert li["block_mode"] == 2, (what, li)
        assert_same(got, full, what + " MaxMatches 1")
        assert st["n_overflow_blocks"] >= 1, what
        probes = set(map(tuple, self.e.overflow_probes().tolist()))
        assert hotm <= probes, (what, len(hotm), len(hotm - probes), sorted(hotm - probes)[:5])
        # the smallest MaxMatches that starts with the screening sketch (host threshold MaxMatches / (planned batches x
        # MAX_GRID) = 2; one batch and the spare one planned).  On the device's full grid the per-workgroup threshold is
        # a few units and a read of the motif (40 acceptances in one block) trips it: the pass repeats with exact counters.
        mm1 = 2 * 2 * MAX_GRID
        c1 = with_mm(c, mm1)
        hot1 = hot_probes(reads, targets, c1, full)
        self.set_knobs(dict(knobs, MUSC_DEBUG_GRID=None))
        got, st, li = self.run(c1, False)
        same_instance(li, "MaxMatches %d" % mm1)
        assert li["block_mode"] == 2 and li["exact_rerun"], (what, li)
        assert_same(got, full, what + " MaxMatches %d" % mm1)
        assert (st["n_overflow_blocks"] >= 1) == bool(hot1), (what, st["n_overflow_blocks"], len(hot1))
        probes = set(map(tuple, self.e.overflow_probes().tolist()))
        assert hot1 <= probes and len(probes - hot1) <= 10 + len(hot1) // 100, (what, len(hot1), len(hot1 - probes), len(probes - hot1))


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
@pytest.mark.parametrize("i", range(len(FUSED)), ids=[c[0] for c in FUSED])
def test_fused_instance(ie, i):
    name, want, knobs, key, W, xm = FUSED[i]
    c, reads, targets, full, hot = build_case(i, key, W, xm, N_FUSED)
    ie.check(name, {"match": want}, knobs, c, reads, targets, full, hot)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(TWO)), ids=[c[0] for c in TWO])
def test_two_kernel_instance(ie, i):
    name, screen, confirm, knobs, key, W, xm = TWO[i]
    c, reads, targets, full, hot = build_case(200 + i, key, W, xm, N_TWO)
    ie.check(name, {"screen": screen, "confirm": confirm}, knobs, c, reads, targets, full, hot)
