"""Window keys wider than 16 bases against the CPU oracle, on every kernel path.

Up to WindowWidth 15 the key is one 32-bit word in a direct table (key_dinucs16, __brev(key), no hash), and that is
where every other module pins its kernel instances.  From 16 on the table is hashed -- bucket_of / rec_bucket fold
the key 64 bits at a time through mix64, the mask plane with it -- the MinDinuc gate is rec_count_dinuc (32-base chunks
that overlap by one base, chunks with and without X merged at the end; 16 itself is the control: one word, hashed,
rec_count_dinuc16), and a window's exact match is taken from masks that span several words (mp.wm / bit_range_mask in
k_match_t and k_match_g, window_word_mask in confirm_pair) -- on a hashed table the only thing that rejects a colliding
key.  Cases, reads and the oracle's tuples: tests/window_key_cases.py (coverage conditions and the agreement of the
two CPU oracles: tests/test_window_key_cases.py).

A run is a case on a path.  Every run asserts FIRST, through stats()["index_kind"], last_instance() and partitions(),
that the pass took the index and launched the instances the run is written for -- a silent fall-back fails -- and then
compares with oracle/literal.cpp's tuples, never with another GPU path, by exact equality of sorted tuple arrays: every
accepted tuple (n_accepted == n_hits == len(oracle), no overflow block), a repeated (sized) pass, best + MMTol 0 and 1,
MatchMode first, and MaxMatches 2, where overflow_probes() names every probe of the oracle's overflowing blocks with at
most 10 + len(hot) // 100 extra (the margin of test_gpu_instances.py; on the 256-bucket tables, where the counters of
unrelated keys are shared, against the probes of the buckets that overflow: window_key_cases.bucket_hot).

Paths: k_match_t on 120-base context buckets in X modes 0, 1, 2 and on wide buckets (two to four windows);
k_match_g<8, 0> (MUSC_MATCH=dma); the two-kernel path under MUSC_INDEX=classic and =lines -- k_screen with and without
the mask plane, k_screen_t<RW>, k_screen<.., lines> under MUSC_SCREEN=wg, k_confirm with two and with three windows --
and where the library takes it by itself (reads that keep the target's X inside a window; the runtime stride: reads of
250 to 450 bases, and 4 200 at WindowWidth 4096); two partitions on a fused and a two-kernel run; and
MUSC_DEBUG_INDEX_BITS=8 on the fused, classic and line paths: 256 buckets hold tens of unrelated entries each, asserted
from n_candidates exceeding the exact candidate count of tests/stats_model.py, so every probe meets colliding keys."""
import os

import pytest

import stats_model as sm
import window_key_cases as wk

pytestmark = pytest.mark.gpu

KNOBS = ("MUSC_INDEX", "MUSC_MATCH", "MUSC_NO_SPEC", "MUSC_DEBUG_CTX_DIRECT", "MUSC_DEBUG_INDEX_BITS", "MUSC_BATCH_READS",
         "MUSC_DEBUG_GRID", "MUSC_CONTEXT", "MUSC_DEBUG_FORCE_WIDE", "MUSC_SCREEN", "MUSC_NO_X_CONTEXT", "MUSC_GRAPH",
         "MUSC_PIPELINE")
# path -> (knobs, partitions); MUSC_DEBUG_GRID=3: one wave of a fused kernel walks several wave-tiles
PATHS = {
    "fused": ({}, False),
    "dma": ({"MUSC_MATCH": "dma"}, False),
    "auto": ({}, False),  # the two-kernel path where the library takes it by itself
    "classic": ({"MUSC_INDEX": "classic"}, False),
    "lines": ({"MUSC_INDEX": "lines"}, False),
    "lines-wg": ({"MUSC_INDEX": "lines", "MUSC_SCREEN": "wg"}, False),
    "fused-bits8": ({"MUSC_DEBUG_INDEX_BITS": "8"}, False),
    "classic-bits8": ({"MUSC_INDEX": "classic", "MUSC_DEBUG_INDEX_BITS": "8"}, False),
    "lines-bits8": ({"MUSC_INDEX": "lines", "MUSC_DEBUG_INDEX_BITS": "8"}, False),
    "fused-parts": ({}, True),
    "classic-parts": ({"MUSC_INDEX": "classic"}, True),
}
ALL_PATHS_WIDTHS = (16, 32, 33, 64)  # every key class, and 33 and 64


def runs():
    out = []
    for name, (ww, wins, L, pm, x) in wk.SPECS.items():
        g = name[0]
        if g == "n" and x == "":
            paths = [p for p in PATHS if p != "auto"] if ww in ALL_PATHS_WIDTHS else ["fused"]
        elif g == "n":
            paths = ["auto", "lines"] if x == "xw" else ["fused", "classic", "lines"]
        elif g == "w":
            paths = ["fused"] + (["classic", "lines"] if name in ("w33", "w64", "w16-3", "w32-3", "w65-3", "w33-4") else [])
        else:
            paths = ["auto", "lines"]
        out.extend((name, p) for p in paths)
    return out


RUNS = runs()


def record_stride(maxlen):
    rw = (-(-2 * maxlen // 32) + 1 + 3) // 4 * 4
    return rw if rw <= 16 else 0  # 0: no instance of its own, the runtime stride


def expected_launch(c, path):
    """-> (index_kind, {"match" / "screen" / "confirm": descriptor}) the run is written for."""
    W, rw = len(c.windows), record_stride(c.lmax)
    span = max(c.windows) - min(c.windows) + c.lmax
    fused = path.split("-")[0] in ("fused", "dma")
    if fused:
        assert c.x in ("", "xr", "xd") and span <= 200 and rw
        wide = int(span > 120)
        if path == "dma":
            return 1, {"match": {"kernel": "k_match_g", "RW": 8, "SG": 0}}
        xm = {"": 0, "xr": 1, "xd": 2}[c.x]
        return 1 + wide, {"match": {"kernel": "k_match_t", "RW": rw, "W": W, "XM": xm, "WIDE": wide, "SG": 0}}
    if path == "auto":
        assert c.x == "xw" or span > 200  # what keeps the run off context buckets
    lines = int(path.startswith("lines"))
    mask, one = int(c.x != ""), int(W <= 2)
    screen = {"kernel": "k_screen", "RW": rw, "mask": mask, "one": one, "lines": lines}
    if lines and not mask and rw and path != "lines-wg":
        screen = {"kernel": "k_screen_t", "RW": rw}
    return 3 * lines, {"screen": screen, "confirm": {"kernel": "k_confirm", "RW": rw, "mask": mask, "w2": one}}


def to_cfg(c, **kw):
    from muscato_amd import Config
    o = c.ocfg(**kw)
    return Config(Windows=list(o.Windows), WindowWidth=o.WindowWidth, PMatch=o.PMatch, MinDinuc=o.MinDinuc,
                  MaxReadLength=o.MaxReadLength, MaxMatches=o.MaxMatches, MMTol=o.MMTol, MatchMode=o.MatchMode)


def assert_same(got, exp, what):
    if got.shape == exp.shape and (got == exp).all():
        return
    g, e = set(map(tuple, got.tolist())), set(map(tuple, exp.tolist()))
    assert False, "%s: gpu %d tuples, oracle %d; missing %s, extra %s" % (what, len(got), len(exp), sorted(e - g)[:5], sorted(g - e)[:5])


class KeyEngine:
    """One Engine for the module: the knobs, database and reads it holds."""

    def __init__(self):
        from muscato_amd import Engine
        self.e = Engine(0)
        self.knobs = None
        self.loaded = None

    def setup(self, knobs, c):
        knobs = dict(knobs, MUSC_DEBUG_GRID="3")
        if knobs != self.knobs:
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update(knobs)
            self.e.reload_env()
            self.knobs, self.loaded = knobs, None  # (a new layout is built over freshly loaded targets)
        if self.loaded != c.name:
            self.e.load_targets(c.targets)
            self.e.load_reads(c.reads)
            self.loaded = c.name
        return self.e

    def run(self, cfg, apply_mmtol):
        from muscato_amd import sorted_hits
        got = sorted_hits(self.e.match(cfg, apply_mmtol=apply_mmtol))
        return got, self.e.stats(), self.e.last_instance()


@pytest.fixture(scope="module")
def ke():
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    s = KeyEngine()
    try:
        yield s
    finally:
        s.e.set_partition_bases(0)
        s.e.close()
        for k in KNOBS:
            os.environ.pop(k, None)
        for k, v in old.items():
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("name,path", RUNS, ids=["%s/%s" % r for r in RUNS])
def test_window_keys(ke, name, path):
    c = wk.case(name)
    exp = wk.oracle_hits(name)
    knobs, parts = PATHS[path]
    kind, want = expected_launch(c, path)
    e = ke.setup(knobs, c)
    what = "%s/%s" % (name, path)

    def launched(st, li, w):
        assert st["index_kind"] == kind, "%s %s: index kind %d, the run is written for %d" % (what, w, st["index_kind"], kind)
        for k in ("match", "screen", "confirm"):
            assert li[k] == want.get(k), "%s %s: launched %s = %s, the run is written for %s" % (what, w, k, li[k], want.get(k))
        assert li["path"] == ("fused" if "match" in want else "two-kernel")
        plan = e.partitions()
        if parts:
            assert len(plan) == 3 and plan[0] == 0 and 0 < plan[1] < plan[2] == len(c.targets), (what, plan)
        else:
            assert plan == [0, len(c.targets)], (what, plan)

    try:
        if parts:
            # two partitions: the cut falls where the first half of the bases ends
            half, acc, cut = c.total_bases // 2, 0, 0
            while acc + len(c.targets[cut]) <= half:
                acc += len(c.targets[cut])
                cut += 1
            assert 0 < cut < len(c.targets) and c.total_bases - acc <= half + max(map(len, c.targets))
            e.set_partition_bases(max(acc, c.total_bases - acc))
        # every accepted tuple
        got, st, li = ke.run(to_cfg(c), False)
        launched(st, li, "all tuples")
        assert_same(got, exp, what + " all tuples")
        print(what, "n_accepted", st["n_accepted"], "n_hits", st["n_hits"], "oracle", len(exp), "n_candidates", st["n_candidates"])
        assert st["n_reads"] == len(c.reads) and st["n_accepted"] == st["n_hits"] == len(exp), (what, st)
        assert st["n_overflow_blocks"] == 0
        if "bits8" in path:
            # 256 buckets: every probe walks unrelated entries, far more than the keys it shares with the database
            model = sm.expected(c.reads, c.targets, c.ocfg(), {0: "classic64", 1: "ctx", 3: "lines"}[kind], exp)
            print(what, "n_candidates", st["n_candidates"], "exact", model["n_candidates"])
            assert st["n_candidates"] > model["n_candidates"], (what, st["n_candidates"], model["n_candidates"])
        # a repeated (sized) pass
        again, st2, li2 = ke.run(to_cfg(c), False)
        launched(st2, li2, "repeated")
        assert_same(again, exp, what + " repeated pass")
        assert st2["n_hits"] == len(exp) and st2["n_overflow_blocks"] == 0
        # best + MMTol
        for mmtol in (0, wk.MMTOL):
            best = wk.best_hits(name, mmtol)
            got, st, li = ke.run(to_cfg(c, MMTol=mmtol), True)
            launched(st, li, "best+%d" % mmtol)
            assert_same(got, best, what + " best + MMTol %d" % mmtol)
            assert st["n_hits"] == len(best) < len(exp) == st["n_accepted"], (what, mmtol, st)
        # MatchMode first
        got, st, li = ke.run(to_cfg(c, MatchMode="first"), False)
        launched(st, li, "first")
        assert_same(got, exp, what + " MatchMode first")
        # MaxMatches 2: the tuples stay, the overflowing blocks' probes are named
        hot = set(wk.hot(name))
        got, st, li = ke.run(to_cfg(c, MaxMatches=wk.SMALL_MM), False)
        launched(st, li, "MaxMatches %d" % wk.SMALL_MM)
        assert li["block_mode"] == 2, (what, li)
        assert_same(got, exp, what + " MaxMatches %d" % wk.SMALL_MM)
        assert st["n_overflow_blocks"] >= 1, what
        probes = set(map(tuple, e.overflow_probes().tolist()))
        print(what, "hot probes", len(hot), "named", len(probes), "extra", len(probes - hot))
        assert hot <= probes, (what, len(hot), sorted(hot - probes)[:5])
        if "bits8" in path:
            # a block counter is keyed by window and BUCKET: in 256 buckets unrelated keys share every counter, and what
            # has to be named are the probes of the buckets whose keys overflow together -- all of them, and the margin
            # on top of those
            hot = wk.bucket_hot(name, 8)
            print(what, "probes of overflowing buckets", len(hot), "extra", len(probes - hot))
            assert hot <= probes, (what, len(hot), sorted(hot - probes)[:5])
        assert len(probes - hot) <= 10 + len(hot) // 100, (what, len(hot), len(probes - hot))
    finally:
        if parts:
            e.set_partition_bases(0)
            ke.loaded = None


def test_window_width_beyond_the_limit_is_refused(ke):
    from muscato_amd import MuscatoError
    c = wk.case("k4096")
    e = ke.setup({}, c)
    cfg = to_cfg(c, WindowWidth=4097, Windows=[1], MaxReadLength=4200)
    with pytest.raises(MuscatoError, match=r"\(2\): bad window_width=4097"):
        e.match(cfg, apply_mmtol=False)
    got, st, li = ke.run(to_cfg(c), False)  # and the context goes on
    assert_same(got, wk.oracle_hits("k4096"), "k4096 after the refused call")
