"""The geometry-specialised fused kernels against the CPU oracle at test size.

SpecGeom<1> (kernels_match_lane_inst.hpp: WindowWidth 15, Windows 0,20, MinDinuc 5, 20 bases of left context, a
DIRECT table of 2^30 buckets) is what BASELINE configs 3 and 4 run by default: k_match_t<8, 2, 0, false, 1>
(match_variant 3) and, with MUSC_MATCH=dma, k_match_g<8, 1> (variant 5).  A database gets that table only from
2^29 bases on, so without help only the whole-cfg3 tests reach these instances -- with 100-base reads, PMatch 0.97
and MaxMatches 10^6 alone.  MUSC_DEBUG_CTX_DIRECT=1 makes the context table direct at any database size: this module
runs the specialised instances on a database of a few Mbp with ragged reads, every PMatch / MMTol / MatchMode of
the grid below and both MaxMatches block modes, checks them against oracle/literal.cpp and against the general
instance on the same table (MUSC_NO_SPEC=1), and asserts match_variant on every pass, so that a silent fall-back
to another kernel (the 2^30-bucket table does not fit: classic index) fails instead of passing.

One Engine per fused kernel holds the 128 GiB table; the tests vary reads and parameters against it, and only the
selection-boundary tests near the end load other geometries.  The fixture closes the engine at teardown, so the
table is gone before the later modules run."""
import os

import numpy as np
import pytest

from oracle import literal
from oracle import muscato_oracle as orc

import stats_model
from cases import hot_probes

pytestmark = pytest.mark.gpu

BATCH = 8192  # MUSC_BATCH_READS: the large read sets take four batches, the last one ragged
SPEC = {"auto": 3, "dma": 5}
GENERAL = {"auto": 2, "dma": 4}
# what the specialised instance reports and what the general instance must report the same
COUNTERS = ("n_read_windows", "n_candidates", "n_pairs", "n_accepted", "n_hits", "n_overflow_entries")
KNOBS = ("MUSC_INDEX", "MUSC_MATCH", "MUSC_NO_SPEC", "MUSC_DEBUG_CTX_DIRECT", "MUSC_DEBUG_INDEX_BITS", "MUSC_BATCH_READS",
         "MUSC_DEBUG_GRID", "MUSC_CONTEXT", "MUSC_DEBUG_FORCE_WIDE")
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
MOTIF_COPIES = 200


def geom(**kw):
    """SpecGeom<1>'s geometry with the given run parameters."""
    c = dict(Windows=[0, 20], WindowWidth=15, PMatch=0.97, MinDinuc=5, MaxReadLength=100, MaxMatches=1000000, MMTol=0)
    c.update(kw)
    return orc.Config(**c)


def _database(seed=5, n_long=2400, tlen=1000, n_short=240):
    """synthetic_medium-style targets (a fifth are copies of others with 2 % substitutions), a 120-base motif planted
    in MOTIF_COPIES of them (heavy (window, key) blocks: a read from the motif has that many placements), and
    targets of 20-99 bases, half of them cut from the motif.  About 2.4 Mbp."""
    rng = np.random.default_rng(seed)
    T = BASES[rng.integers(0, 4, size=(n_long, tlen))]
    ncopy = n_long // 5
    T[n_long - ncopy:] = T[rng.integers(0, n_long - ncopy, size=ncopy)]
    sub = rng.random((ncopy, tlen)) < 0.02
    T[n_long - ncopy:][sub] = BASES[rng.integers(0, 4, size=int(sub.sum()))]
    motif = BASES[rng.integers(0, 4, size=120)]
    for i in rng.choice(n_long - ncopy, size=MOTIF_COPIES, replace=False):
        p = int(rng.integers(0, tlen - 120 + 1))
        T[i, p:p + 120] = motif
    targets = [bytes(t) for t in T]
    for i in range(n_short):
        n = int(rng.integers(20, 100))
        if i % 2:
            o = int(rng.integers(0, 120 - n + 1))
            targets.append(bytes(motif[o:o + n]))
        else:
            targets.append(bytes(BASES[rng.integers(0, 4, size=n)]))
    return targets, bytes(motif)


TARGETS, MOTIF = _database()
_GBUF = literal.concat(TARGETS)


def mutate(rng, s, rate):
    a = np.frombuffer(s, dtype=np.uint8).copy()
    sub = rng.random(len(a)) < rate
    a[sub] = BASES[rng.integers(0, 4, size=int(sub.sum()))]
    return bytes(a)


def reads_of(seed, lens, sub=0.01, rand=0.15, motif=0.02, edge=0.05, targets=None):
    """One read per entry of `lens`: random bases (`rand`), from the motif (`motif`: hundreds of placements each),
    else from a target long enough, at position 0 or flush with its end with probability `edge` each.
    Sorted and unique, as the library's loaders are fed; the count is never a multiple of 64."""
    rng = np.random.default_rng(seed)
    targets = TARGETS if targets is None else targets
    tl = np.array([len(t) for t in targets])
    out = set()
    for L in lens:
        L = int(L)
        u = rng.random()
        if u < rand:
            out.add(bytes(BASES[rng.integers(0, 4, size=L)]))
            continue
        if u < rand + motif and L <= len(MOTIF):
            o = int(rng.integers(0, len(MOTIF) - L + 1))
            out.add(mutate(rng, MOTIF[o:o + L], sub))
            continue
        fit = np.flatnonzero(tl >= L)
        g = int(fit[rng.integers(0, len(fit))])
        v = rng.random()
        p = 0 if v < edge else int(tl[g]) - L if v < 2 * edge else int(rng.integers(0, tl[g] - L + 1))
        out.add(mutate(rng, targets[g][p:p + L], sub))
    reads = sorted(out)
    if len(reads) % 64 == 0:
        reads = reads[:-1]
    return reads


def ragged_lengths(rng, n):
    """Every length class the specialised instance treats apart: below 15 (no window), 15-34 (window 0 only),
    35-84, 85 / 86 (either side of the literal-100 rule at position 0), 87-99 and exactly 100."""
    return rng.choice(np.r_[np.arange(5, 15), np.arange(15, 35), np.arange(35, 85), [85, 86] * 10, np.arange(87, 100),
                            [99] * 10, [100] * 40], size=n)


def oracle_full(reads, c, targets=None):
    """Every accepted tuple (no MaxMatches truncation: the literal port with a limit no block reaches keeps what
    orc.match_direct(..., check_overflow=False) returns)."""
    gbuf, goff = _GBUF if targets is None else literal.concat(targets)
    rbuf, roff = literal.concat(reads)
    big = orc.Config(**dict(c.__dict__, MaxMatches=2 ** 31 - 1))
    exp, _, _ = literal.match_arrays(rbuf, roff, gbuf, goff, literal.make_params(big, bloom_size=64_000_000, num_hash=8, nthreads=8))
    return exp


def oracle_hot_probes(reads, c, full, targets=None):
    return hot_probes(reads, TARGETS if targets is None else targets, c, full)


def to_cfg(c):
    from muscato_amd import Config
    return Config(Windows=list(c.Windows), WindowWidth=c.WindowWidth, PMatch=c.PMatch, MinDinuc=c.MinDinuc,
                  MaxReadLength=c.MaxReadLength, MaxMatches=c.MaxMatches, MMTol=c.MMTol, MatchMode=c.MatchMode)


def assert_same(got, exp, what=""):
    assert got.shape == exp.shape, "%s: hit count differs: gpu %d vs oracle %d" % (what, len(got), len(exp))
    assert (got == exp).all(), what


class SpecEngine:
    """One Engine with the SpecGeom<1> table resident, and the read set and database it holds."""

    def __init__(self, mode):
        from muscato_amd import Engine
        self.mode = mode
        self.e = Engine(0)
        self.targets = None
        self.reads = None
        self.load_targets(TARGETS)

    def load_targets(self, targets):
        if self.targets is not targets:
            self.e.load_targets(targets)
            self.targets = targets
            self.reads = None

    def load_reads(self, reads):
        if self.reads is not reads:
            self.e.load_reads(reads)
            self.reads = reads

    def knob(self, name, value):
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value
        self.e.reload_env()

    def run(self, reads, c, apply_mmtol):
        from muscato_amd import sorted_hits
        self.load_reads(reads)
        got = sorted_hits(self.e.match(to_cfg(c), apply_mmtol=apply_mmtol))
        return got, self.e.stats()

    def check(self, reads, c, variant="spec", general=True, exp=None, what="", model=False):
        """Full tuple set and best+MMTol selection against the oracle, the kernel variant on both passes, and (spec,
        general=True) the general instance on the same table: identical tuples and counters.  model=True: the
        counters and the algorithmic bytes also equal tests/stats_model.py's (the table is direct and the reads hold no
        X: equalities), which ties the specialised instance to the oracle's own count and not only to the general
        instance.  -> (tuples, stats)."""
        what = "%s %s %s" % (self.mode, what, c)
        full = oracle_full(reads, c, self.targets if self.targets is not TARGETS else None) if exp is None else exp
        want = (SPEC if variant == "spec" else GENERAL)[self.mode] if variant in ("spec", "general") else variant
        got, st = self.run(reads, c, False)
        assert st["index_kind"] == 1, what
        assert st["match_variant"] == want, (what, st["match_variant"])
        assert_same(got, full, what)
        if model:
            want_st = model_counters(reads, self.targets, c, full)
            for k in COUNTERS + MODEL_BYTES:
                assert st[k] == want_st[k], (what, "model", k, st[k], want_st[k])
            assert st["n_descriptors"] == 0 and st["match_launches"] == st["n_batches"] == (len(reads) + BATCH - 1) // BATCH, what
        best, st2 = self.run(reads, c, True)
        assert st2["match_variant"] == want, (what, st2["match_variant"])
        assert_same(best, np.array(sorted(orc.best_filter(map(tuple, full.tolist()), c.MMTol)), dtype=np.uint32).reshape(-1, 4),
                    what + " best+MMTol")
        if variant == "spec" and general:
            self.knob("MUSC_NO_SPEC", "1")
            try:
                got2, gst = self.run(reads, c, False)
            finally:
                self.knob("MUSC_NO_SPEC", None)
            assert gst["match_variant"] == GENERAL[self.mode], what
            assert gst["ms_index_build"] == st["ms_index_build"], what  # MUSC_NO_SPEC does not rebuild the table
            assert_same(got2, got, what + " general instance")
            for k in COUNTERS + ("n_overflow_blocks",):
                assert gst[k] == st[k], (what, k, gst[k], st[k])
            if model:
                for k in COUNTERS + MODEL_BYTES:
                    assert gst[k] == want_st[k], (what, "model, general instance", k, gst[k], want_st[k])
        return full, st


MODEL_BYTES = ("match_bytes", "match_bytes_strict")
_MODEL = {}


def model_counters(reads, targets, c, full):
    """tests/stats_model.py's counters for narrow context buckets, once per read set (both fused kernels ask)."""
    key = (id(reads), id(targets), str(c))
    if key not in _MODEL:
        _MODEL[key] = (stats_model.expected(reads, targets, c, "ctx", full), reads, targets)
    return _MODEL[key][0]


_PROBES = {}  # mode -> (reads, config, the specialised instance's overflow probes): the classic path's check at the end


@pytest.fixture(scope="module", params=["auto", "dma"])
def se(request):
    """The specialised instance of k_match_t (auto) or of k_match_g (MUSC_MATCH=dma) on a direct 2^30-bucket table."""
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ["MUSC_DEBUG_CTX_DIRECT"] = "1"
    os.environ["MUSC_BATCH_READS"] = str(BATCH)
    if request.param == "dma":
        os.environ["MUSC_MATCH"] = "dma"
    s = SpecEngine(request.param)
    try:
        yield s
    finally:
        s.e.close()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_uniform_100_base_reads(se):
    """(a) every read 100 bases: the constant-mask tiles.  Three full batches and a ragged fourth.  The counters and
    bytes of the specialised and of the general instance equal the CPU model's."""
    reads = _uniform_reads()
    assert len(reads) > 3 * BATCH
    full, _ = se.check(reads, geom(), model=True)
    assert len(full) > 20000


_UNIFORM = []


def _uniform_reads():
    if not _UNIFORM:
        _UNIFORM.append(reads_of(1, [100] * 30000))
    return _UNIFORM[0]


@pytest.mark.parametrize("L", [80, 49, 99])
def test_uniform_length_other_than_100(se, L):
    """(b) tiles of one length that is not the geometry's: the host's per-length mask rows (mp->lm)."""
    reads = reads_of(2 + L, [L] * 20000)
    full, _ = se.check(reads, geom(MaxReadLength=L))
    assert len(full) > 10000


def test_ragged_lengths(se):
    """(c) every length class in one set: wave-tiles of mixed lengths, per-lane length masks."""
    rng = np.random.default_rng(3)
    reads = reads_of(3, ragged_lengths(rng, 30000))
    lens = {len(r) for r in reads}
    assert min(lens) < 15 and {15, 34, 35, 84, 85, 86, 99, 100} <= lens
    full, _ = se.check(reads, geom())
    assert len(full) > 10000


@pytest.mark.parametrize("n", [1, 7, 63, 65, 127, 1000])
def test_read_counts(se, n):
    """(d) read sets of fewer than 64 reads and counts that are not a multiple of 64 (a partial last wave-tile)."""
    rng = np.random.default_rng(100 + n)
    lens = ragged_lengths(rng, 4 * n)
    lens[:4] = 100
    pool = reads_of(100 + n, lens, rand=0.05)
    long = [r for r in pool if len(r) == 100][:1]  # (every window has a read long enough for it)
    reads = sorted(long + [r for r in pool if r not in long][:n - 1])
    assert len(reads) == n
    se.check(reads, geom(PMatch=0.95, MMTol=1))


def test_placement_edges(se):
    """Reads at target position 0 and flush with the target end, 80-90 bases long (the literal-100 rule: at jx = 0 a
    read of more than 85 bases does not fit window 0), with window 1 or window 0 mutated so that only the other
    window finds them; reads whose window 1 matches a target at jx < 20 (position < 0: no placement); whole short
    targets as reads."""
    rng = np.random.default_rng(4)
    out = set()
    long_t = [t for t in TARGETS if len(t) >= 100]
    for i in range(12000):
        L = int(rng.integers(80, 91))
        t = long_t[int(rng.integers(0, len(long_t)))]
        kind = i % 4
        if kind == 0:    # position 0, window 1 broken: only window 0 (jx = 0) can place it
            r = bytearray(t[:L])
            j = 20 + int(rng.integers(0, 15))
            r[j] = b"ACGT"[(b"ACGT".index(r[j]) + 1) % 4]
            out.add(bytes(r))
        elif kind == 1:  # position 0, as it is
            out.add(mutate(rng, t[:L], 0.01))
        elif kind == 2:  # flush with the end, window 0 broken for half of them
            r = bytearray(t[len(t) - L:])
            if i % 8 == 2:
                j = int(rng.integers(0, 15))
                r[j] = b"ACGT"[(b"ACGT".index(r[j]) + 1) % 4]
            out.add(bytes(r))
        else:            # window 1 = target bases from jx = 20 - d < 20
            d = int(rng.integers(1, 20))
            out.add(bytes(BASES[rng.integers(0, 4, size=d)]) + t[:L - d])
    out |= {t for t in TARGETS if len(t) < 100}
    reads = sorted(out)
    c = geom(PMatch=0.95, MMTol=3)
    full, _ = se.check(reads, c)
    zero = {p for _, _, p, _ in full.tolist()}
    assert 0 in zero and len(full) > 5000


# PMatch x MMTol x MatchMode, pairwise
GRID = [(pm, mm, ("best", "first")[(i + j) % 2]) for i, pm in enumerate((1.0, 0.97, 0.95, 0.9, 0.8)) for j, mm in enumerate((0, 1, 3))]


@pytest.mark.parametrize("pmatch,mmtol,mode", GRID)
def test_parameter_grid(se, pmatch, mmtol, mode):
    """Mismatch budgets of other PMatch values (nmiss_tab), MMTol and the best selection, MatchMode, on ragged reads
    with 3 % substitutions (hits at every budget)."""
    reads = _grid_reads()
    c = geom(PMatch=pmatch, MMTol=mmtol, MatchMode=mode)
    full, _ = se.check(reads, c)
    assert len(full) > 5000


_GRID_READS = []


def _grid_reads():
    if not _GRID_READS:
        _GRID_READS.append(reads_of(7, ragged_lengths(np.random.default_rng(7), 25000), sub=0.03))
    return _GRID_READS[0]


def _motif_reads(n, seed):
    """n reads of 60-100 bases from motif offset 0 with substitutions outside window 0: one (window 0, key) block of
    about n x MOTIF_COPIES accepted pairs."""
    rng = np.random.default_rng(seed)
    out = set()
    while len(out) < n:
        L = int(rng.integers(60, 101))
        out.add(MOTIF[:15] + mutate(rng, MOTIF[15:L], 0.03))
    return sorted(out)


def test_maxmatches(se):
    """MaxMatches accounting on heavy blocks.  A small MaxMatches gives block_mode 2 (exact counters) at once;
    20 000 on 1 000 reads (two planned batches: threshold 20000 / (2 x MAX_GRID) = 2, and per resident workgroup
    higher) starts in block_mode 1, where one read of the motif (200 acceptances in one block) trips any workgroup's
    screen into the exact re-run; 41 000 on the ragged 30 000-read set (five planned batches) the same without an
    overflow; 10^6.  Tuples: every accepted one (the oracle without truncation).  n_overflow_blocks >= 1 exactly when an
    oracle block overflows; overflow_probes() names at least the oracle's hot probes and the same ones as the general
    instance."""
    ragged = reads_of(3, ragged_lengths(np.random.default_rng(3), 30000))
    heavy = _motif_reads(1000, 8)
    cases = [(ragged, 5, True), (ragged, 25, True), (heavy, 20000, True), (ragged, 41000, False), (ragged, 1000000, False)]
    for reads, mm, overflows in cases:
        c = geom(MaxMatches=mm, MMTol=1)
        full = oracle_full(reads, c)
        hot = oracle_hot_probes(reads, c, full)
        assert bool(hot) == overflows, (mm, len(hot))
        _, st = se.check(reads, c, exp=full, what="MaxMatches %d" % mm)
        assert (st["n_overflow_blocks"] >= 1) == overflows, (mm, st["n_overflow_blocks"])
        probes = set(map(tuple, se.e.overflow_probes().tolist()))
        assert hot <= probes and len(probes - hot) <= 10 + len(hot) // 100, (mm, len(hot - probes), len(probes - hot))
        se.knob("MUSC_NO_SPEC", "1")
        try:
            _, gst = se.run(reads, c, False)
            gprobes = set(map(tuple, se.e.overflow_probes().tolist()))
        finally:
            se.knob("MUSC_NO_SPEC", None)
        assert gst["match_variant"] == GENERAL[se.mode]
        assert gprobes == probes, mm
        if mm == 25:
            _PROBES[se.mode] = (reads, c, probes)


def test_selection_boundaries(se):
    """With the knob on, the specialised instance runs exactly where its geometry and record layout hold: reads of at
    most 48 bases take 4-word records (general k_match_t: k_match_g exists for 8-word records only), 49 and 100 take 8
    (specialised), 101 wide buckets (general k_match_t); MinDinuc 4: general; X in the reads: general k_match_t.
    Every one equals the oracle."""
    rng = np.random.default_rng(9)
    for L, variant in ((48, 2), (49, "spec"), (100, "spec")):
        lens = rng.integers(15, L + 1, size=6000)
        lens[:50] = L
        reads = reads_of(900 + L, lens)
        assert max(map(len, reads)) == L
        se.check(reads, geom(MaxReadLength=L), variant=variant, what="max length %d" % L)
    reads = reads_of(10, ragged_lengths(rng, 8000))
    se.check(reads, geom(MinDinuc=4), variant="general", what="MinDinuc 4")
    # one X per read: every read lists its X in its xpos word, so the run stays on the context table (k_match_t)
    xr = []
    for r in reads:
        b = bytearray(r)
        if len(b) > 40 and rng.random() < 0.3:
            b[int(rng.integers(0, len(b)))] = ord("X")
        xr.append(bytes(b))
    xr = sorted(set(xr))
    se.check(xr, geom(), variant=2, what="X in the reads")
    # 101 bases: wide buckets (a rebuild), the general instance of k_match_t
    lens = rng.integers(40, 102, size=6000)
    lens[:20] = 101
    reads = reads_of(11, lens)
    full = oracle_full(reads, geom(MaxReadLength=101))
    got, st = se.run(reads, geom(MaxReadLength=101), False)
    assert st["index_kind"] == 2 and st["match_variant"] == 2
    assert_same(got, full, "101 bases")


def test_other_geometries_and_the_knob(se):
    """One step off the geometry -- Windows 0,21 (20 + 1 bases of context), WindowWidth 14 (a direct 2^28 table) --
    runs the general instance.  Then the knob itself: MUSC_DEBUG_CTX_DIRECT unset through reload_env gives this
    database its ordinary hashed table (the resident table's kind is part of ensure_index's comparison, so the
    table is rebuilt) and the general instance; set again, the direct table and the specialised one."""
    rng = np.random.default_rng(12)
    reads = reads_of(12, rng.integers(40, 100, size=8000))
    se.check(reads, geom(Windows=[0, 21], MaxReadLength=99), variant="general", what="Windows 0,21")
    se.check(reads, geom(WindowWidth=14), variant="general", what="WindowWidth 14")
    c = geom(PMatch=0.95, MMTol=1)
    full = oracle_full(reads, c)
    se.knob("MUSC_DEBUG_CTX_DIRECT", None)
    try:
        se.check(reads, c, variant="general", exp=full, what="hashed table")
    finally:
        se.knob("MUSC_DEBUG_CTX_DIRECT", "1")
    se.check(reads, c, exp=full, what="direct table again")


def test_database_with_x(se):
    """X in the database: the general instance on the direct table (k_match_t<.., XM = 2>), equal to the oracle.  (The
    reads are drawn from the X-free targets: a read with an X in one of its windows would send the run to the
    two-kernel path, reads_x_fit_db.)"""
    rng = np.random.default_rng(13)
    xt = list(TARGETS)
    for i in range(0, len(xt), 7):
        t = bytearray(xt[i])
        t[int(rng.integers(0, len(t)))] = ord("X")
        xt[i] = bytes(t)
    reads = reads_of(13, ragged_lengths(rng, 8000))
    se.load_targets(xt)
    try:
        se.check(reads, geom(PMatch=0.95, MMTol=1), variant=2, what="database with X")
    finally:
        se.load_targets(TARGETS)


def test_zz_classic_path_names_the_same_overflow_probes(se):
    """The two-kernel path (MUSC_INDEX=classic) on the MaxMatches 25 case of test_maxmatches: the same tuples, and both
    paths name every probe of an overflowing block.  The exact block counters are a 2^22-cell table hashed by
    (window, bucket number), and the two paths number buckets differently (the key itself on the direct context
    table, a hashed window-start bucket on the classic one): a key that shares a cell with an overflowing block is
    reported too, and such extras differ between the paths.  They stay a handful.  Last in the module: the classic
    index drops the context table."""
    assert se.mode in _PROBES, "test_maxmatches did not run"
    reads, c, probes = _PROBES[se.mode]
    full = oracle_full(reads, c)
    hot = oracle_hot_probes(reads, c, full)
    se.knob("MUSC_INDEX", "classic")
    try:
        got, st = se.run(reads, c, False)
        cprobes = set(map(tuple, se.e.overflow_probes().tolist()))
    finally:
        se.knob("MUSC_INDEX", None)
    assert st["index_kind"] == 0 and st["match_variant"] == 0
    assert_same(got, full, "classic")
    assert st["n_overflow_blocks"] >= 1 and hot <= cprobes and hot <= probes
    assert len(cprobes - hot) + len(probes - hot) <= 10 + len(hot) // 100, (len(hot), len(cprobes - hot), len(probes - hot))
