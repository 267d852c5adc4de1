"""A database matched in partitions (musc_db_set_partition_bases, the automatic planner) against the unpartitioned
pass on the same engine setup and against the literal oracle: the same tuples (every accepted one, and the GLOBAL
best + MMTol selection), a read-major list that musc_hits_copy_compact accepts, the whole-database MaxMatches verdict
and the reported plan -- on every index path (context buckets with k_match_t / k_match_g / the specialised instance,
64-byte and line buckets)."""
import os

import numpy as np
import pytest

from oracle import literal
from oracle import muscato_oracle as orc

from cases import hot_probes

pytestmark = pytest.mark.gpu

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
KNOBS = ("MUSC_INDEX", "MUSC_MATCH", "MUSC_DEBUG_CTX_DIRECT", "MUSC_GRAPH", "MUSC_DEBUG_INDEX_BUDGET_MB", "MUSC_BATCH_READS")
PATHS = {  # environment -> (index_kind values it may report, match_variant it must report: None = any)
    "default": ({}, (1,), 2),
    "dma": ({"MUSC_MATCH": "dma"}, (1,), 4),  # k_match_g: no X on either side (TARGETS_NOX)
    "classic": ({"MUSC_INDEX": "classic"}, (0, 3), 0),
    "lines": ({"MUSC_INDEX": "lines"}, (3,), 0),
    "ctx_direct": ({"MUSC_DEBUG_CTX_DIRECT": "1"}, (1,), 3),  # SpecGeom<1>: no X, MinDinuc 5
}
NO_X = ("dma", "ctx_direct")


def _database(seed=11):
    """Ragged targets: some shorter than the window, a few long ones, some with an X; about 90 kbp."""
    rng = np.random.default_rng(seed)
    lens = np.r_[rng.integers(3, 15, 8), rng.integers(100, 2500, 50), rng.integers(4000, 9000, 6)]
    rng.shuffle(lens)
    out = []
    for i, n in enumerate(lens):
        t = BASES[rng.integers(0, 4, int(n))].copy()
        if i % 9 == 4 and n > 50:
            t[int(rng.integers(0, n))] = ord("N")
        out.append(bytes(t))
    return out


TARGETS = _database()
TARGETS_NOX = [t.replace(b"N", b"A") for t in TARGETS]  # k_match_g and the specialised instance: no X on either side
NB = sum(len(t) for t in TARGETS)


def mutate(rng, s, rate):
    a = np.frombuffer(s, dtype=np.uint8).copy()
    sub = rng.random(len(a)) < rate
    a[sub] = BASES[rng.integers(0, 4, size=int(sub.sum()))]
    return bytes(a)


def reads_of(seed, n, lens=(40, 100), targets=TARGETS, fixed=None):
    rng = np.random.default_rng(seed)
    tl = np.array([len(t) for t in targets])
    out = set()
    for _ in range(n):
        L = fixed or int(rng.integers(lens[0], lens[1] + 1))
        if rng.random() < 0.15:
            out.add(bytes(BASES[rng.integers(0, 4, L)]))
            continue
        fit = np.flatnonzero(tl >= L)
        g = int(fit[rng.integers(0, len(fit))])
        p = int(rng.integers(0, tl[g] - L + 1))
        s = targets[g][p:p + L].replace(b"N", b"A")
        out.add(mutate(rng, s, 0.03))
    return sorted(out)


READS = reads_of(3, 1500)


def ocfg(**kw):
    c = dict(Windows=[0, 20], WindowWidth=15, PMatch=0.9, MinDinuc=0, MaxReadLength=100, MaxMatches=1000000, MMTol=0)
    c.update(kw)
    return orc.Config(**c)


def to_cfg(c):
    from muscato_amd import Config
    return Config(Windows=list(c.Windows), WindowWidth=c.WindowWidth, PMatch=c.PMatch, MinDinuc=c.MinDinuc,
                  MaxReadLength=c.MaxReadLength, MaxMatches=c.MaxMatches, MMTol=c.MMTol, MatchMode=c.MatchMode)


def oracle_full(reads, targets, c):
    gbuf, goff = literal.concat(targets)
    rbuf, roff = literal.concat(reads)
    big = orc.Config(**dict(c.__dict__, MaxMatches=2 ** 31 - 1))
    exp, _, _ = literal.match_arrays(rbuf, roff, gbuf, goff, literal.make_params(big, bloom_size=16_000_000, num_hash=8, nthreads=8))
    return exp


def best_of(full, mmtol):
    return np.array(sorted(orc.best_filter(map(tuple, full.tolist()), mmtol)), dtype=np.uint32).reshape(-1, 4)


def srt(a):
    from muscato_amd import sorted_hits
    return sorted_hits(a)


def set_env(env):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)


@pytest.fixture
def engine_for():
    made = []

    def make(env):
        from muscato_amd import Engine
        set_env(env)
        try:
            e = Engine(0)
        finally:
            set_env({})
        made.append(e)
        return e

    yield make
    for e in made:
        e.close()


def raw_hits(e, c, apply_mmtol):
    n = e.match_device(to_cfg(c), apply_mmtol=apply_mmtol)
    out = np.zeros((n, 4), dtype=np.uint32)
    if n:
        e.hits_to(out.ctypes.data, n, False)
    return out


def check_read_major(e, hits):
    """reads increasing, each read's tuples contiguous; musc_hits_copy_compact accepts the list and decodes to it"""
    assert (np.diff(hits[:, 0].astype(np.int64)) >= 0).all()
    n, nr = len(hits), e.n_reads
    words = np.zeros(max(n, 1), np.uint32)
    counts = np.zeros(max(nr, 1), np.uint8)
    bits = (8, 18, 6)
    e.hits_to_compact(words.ctypes.data, n, counts.ctypes.data, nr, False, bits)
    assert int(counts[:nr].sum()) == n
    reads = np.repeat(np.arange(nr, dtype=np.uint32), counts[:nr])
    dec = np.stack([reads, words[:n] >> 24, (words[:n] >> 6) & 0x3FFFF, words[:n] & 63], axis=1).astype(np.uint32)
    assert (dec == hits).all()


LIMITS = {"one_target": 1, "two": (NB + 1) // 2, "three": (NB + 2) // 3, "below_longest": 3000}


@pytest.mark.parametrize("path", list(PATHS))
def test_partitioned_equals_unpartitioned_and_oracle(engine_for, path):
    env, kinds, variant = PATHS[path]
    e = engine_for(env)
    targets = TARGETS_NOX if path in NO_X else TARGETS
    e.load_targets(targets)
    e.load_reads(READS)
    md = 5 if path == "ctx_direct" else 0  # (SpecGeom<1>: MinDinuc 5)
    grid = [ocfg(PMatch=0.9, MMTol=0, MinDinuc=md), ocfg(PMatch=0.95, MMTol=2, MatchMode="first", MinDinuc=md),
            ocfg(PMatch=1.0, MMTol=1, MinDinuc=md), ocfg(PMatch=0.92, MMTol=3, MinDinuc=md)]
    limits = dict(LIMITS)
    if path == "ctx_direct":  # (a 2^30-bucket table per partition: the coarse plans only)
        limits = {k: v for k, v in limits.items() if k in ("two", "three")}
    for c in grid:
        full = oracle_full(READS, targets, c)
        best = best_of(full, c.MMTol)
        e.set_partition_bases(0)
        ref = {a: srt(raw_hits(e, c, a)) for a in (False, True)}
        st0 = e.stats()
        assert e.partitions() == [0, len(TARGETS)]
        assert st0["match_variant"] == variant, (path, st0)
        assert (ref[False] == full).all() and (ref[True] == best).all(), (path, c)
        for name, lim in limits.items():
            e.set_partition_bases(lim)
            for a in (False, True):
                got = raw_hits(e, c, a)
                st = e.stats()
                plan = e.partitions()
                assert len(plan) > 2 and plan[0] == 0 and plan[-1] == len(TARGETS), (path, name, plan)
                if name == "one_target":
                    assert len(plan) == len(TARGETS) + 1
                assert st["index_kind"] in kinds and st["index_kind"] == st0["index_kind"], (path, name, st)
                assert st["match_variant"] == variant, (path, name, st)
                check_read_major(e, got)
                assert srt(got).shape == ref[a].shape and (srt(got) == ref[a]).all(), (path, name, c, a)
                assert st["n_hits"] == len(got) and st["n_overflow_blocks"] == 0
    e.set_partition_bases(0)


def test_build_index_for_builds_the_first_partition(engine_for):
    """musc_db_build_index_for under a partition limit plans the pass and builds partition 0's index; the match that
    follows gives the unpartitioned tuples."""
    c = ocfg(PMatch=0.95, MMTol=1)
    e = engine_for({})
    e.load_targets(TARGETS)
    e.load_reads(READS)
    ref = srt(raw_hits(e, c, True))
    e.set_partition_bases((NB + 1) // 2)
    e.build_index_for(to_cfg(c), 100)
    plan = e.partitions()
    assert len(plan) > 2 and plan[-1] == len(TARGETS)
    got = raw_hits(e, c, True)
    assert e.partitions() == plan
    check_read_major(e, got)
    assert (srt(got) == ref).all()
    # and back to the automatic plan: one partition, the whole-database index
    e.set_partition_bases(0)
    e.build_index_for(to_cfg(c), 100)
    assert e.partitions() == [0, len(TARGETS)]
    assert (srt(raw_hits(e, c, True)) == ref).all()


def test_global_best_in_a_later_partition(engine_for):
    """The read's exact placement is in the last partition; the earlier partition holds 2- and 3-mismatch placements,
    within its own best + MMTol but not within the global one: they must go."""
    rng = np.random.default_rng(7)
    core = bytes(BASES[rng.integers(0, 4, 60)])
    def sub(s, where):
        a = bytearray(s)
        for p in where:
            a[p] = ord("A") if a[p] != ord("A") else ord("C")
        return bytes(a)
    pad = lambda: bytes(BASES[rng.integers(0, 4, 200)])
    targets = [pad() + sub(core, [45, 50]) + pad(), pad() + sub(core, [41, 47, 55]) + pad(), pad(), pad() + core + pad()]
    e = engine_for({})
    e.load_targets(targets)
    e.load_reads([core])
    c = ocfg(PMatch=0.9, MMTol=1)
    e.set_partition_bases(0)
    whole = srt(e.match(to_cfg(c), apply_mmtol=True))
    assert whole.tolist() == [[0, 3, 200, 0]]
    e.set_partition_bases(930)
    got = raw_hits(e, c, True)
    assert e.partitions() == [0, 2, 4]
    assert got.tolist() == [[0, 3, 200, 0]]
    allh = srt(raw_hits(e, c, False))
    assert sorted(allh[:, 3].tolist()) == [0, 2, 3]


def test_maxmatches_block_split_over_partitions(engine_for):
    """A (window, key) block of 12 accepted placements, 6 in each partition, with MaxMatches 10: the verdict is the
    whole database's, and the probes include the unpartitioned ones."""
    rng = np.random.default_rng(9)
    read = bytes(BASES[rng.integers(0, 4, 50)])
    targets = [bytes(BASES[rng.integers(0, 4, 30)]) + read + bytes(BASES[rng.integers(0, 4, 30)]) for _ in range(12)]
    e = engine_for({})
    e.load_targets(targets)
    reads = sorted({read} | set(reads_of(5, 40, lens=(40, 60), targets=targets)))
    e.load_reads(reads)
    c = ocfg(PMatch=0.9, MaxMatches=10, MaxReadLength=60)
    e.set_partition_bases(0)
    ref = srt(raw_hits(e, c, False))
    st0 = e.stats()
    pr0 = {tuple(p) for p in e.overflow_probes().tolist()}
    assert st0["n_overflow_blocks"] > 0 and pr0
    assert pr0 >= hot_probes(reads, targets, c, oracle_full(reads, targets, c))
    e.set_partition_bases(6 * len(targets[0]))
    got = raw_hits(e, c, False)
    assert len(e.partitions()) == 3
    st = e.stats()
    assert st["n_overflow_blocks"] > 0
    assert {tuple(p) for p in e.overflow_probes().tolist()} >= pr0
    assert (srt(got) == ref).all()
    # the core read alone: 6 accepted pairs per window in each partition, 12 in all -- only the summed counters see it
    e.load_reads([read])
    raw_hits(e, c, False)
    assert len(e.partitions()) == 3 and e.stats()["n_overflow_blocks"] > 0
    assert {tuple(p) for p in e.overflow_probes().tolist()} == {(0, 0), (0, 1)}
    e.set_partition_bases(0)
    e.load_targets(targets[:6])
    raw_hits(e, c, False)
    assert e.stats()["n_overflow_blocks"] == 0


def test_async_upload_repeat_and_graph(engine_for):
    """musc_reads_load_packed32(async) feeds the first partition; two identical calls in a row and MUSC_GRAPH=1 give
    the same list."""
    from muscato_amd.api import pack_2bit, concat
    reads = reads_of(21, 3000, fixed=100)
    c = ocfg(PMatch=0.95, MMTol=1)
    exp = best_of(oracle_full(reads, TARGETS, c), c.MMTol)
    for env in ({"MUSC_BATCH_READS": "512"}, {"MUSC_GRAPH": "1"}):
        e = engine_for(env)
        e.load_targets(TARGETS)
        e.set_partition_bases((NB + 2) // 3)
        buf, off = concat(reads)
        packed, mask = pack_2bit(buf, int(off[-1]))
        assert mask is None
        packed = np.concatenate([packed, np.zeros(8, np.uint8)])
        e.load_reads_packed32_ptr(packed.ctypes.data, 0, 0, 100, len(reads), True)
        first = raw_hits(e, c, True)
        second = raw_hits(e, c, True)
        third = raw_hits(e, c, True)
        assert len(e.partitions()) > 3
        check_read_major(e, first)
        assert (srt(first) == exp).all()
        assert (first == second).all() and (second == third).all()


def test_automatic_plan_under_an_index_budget(engine_for):
    """MUSC_DEBUG_INDEX_BUDGET_MB makes the automatic planner split a database of ~24 Mbp (no index kind of the whole
    database fits 1500 MiB); the tuples equal the unbudgeted pass's."""
    rng = np.random.default_rng(5)
    targets = [bytes(BASES[rng.integers(0, 4, int(n))]) for n in rng.integers(50_000, 150_000, 240)]
    reads = reads_of(8, 4000, lens=(80, 100), targets=targets)
    c = ocfg(PMatch=0.95, MMTol=1)
    plain = engine_for({})
    plain.load_targets(targets)
    plain.load_reads(reads)
    ref = {a: srt(raw_hits(plain, c, a)) for a in (False, True)}
    assert plain.partitions() == [0, len(targets)]
    plain.close()
    e = engine_for({"MUSC_DEBUG_INDEX_BUDGET_MB": "1500"})
    e.load_targets(targets)
    e.load_reads(reads)
    for a in (False, True):
        got = raw_hits(e, c, a)
        assert len(e.partitions()) > 2, e.partitions()
        check_read_major(e, got)
        assert (srt(got) == ref[a]).all()
    assert e.stats()["index_kind"] == 0  # (1500 MiB: neither context table fits; 64-byte buckets of half the database do)


def test_resident_window_index_survives_an_unfitting_context_table(engine_for):
    """Context buckets are eligible but do not fit (WindowWidth 15 over 116 182 bases under 15 MiB: the hashed context
    table needs 19 899 300 B, 64-byte buckets 12 344 752 B), so the pass runs on the window-start index -- and later
    passes with the same parameters find it resident.  stats()["ms_index_build"] is kept across passes and rewritten
    only by a build (a fresh event time), so it stays bit-equal exactly when nothing was rebuilt."""
    c = ocfg(PMatch=0.95, MMTol=1)
    full = oracle_full(READS, TARGETS_NOX, c)
    e = engine_for({"MUSC_DEBUG_INDEX_BUDGET_MB": "15"})
    e.load_targets(TARGETS_NOX)
    e.load_reads(READS)
    first = srt(raw_hits(e, c, False))
    st = e.stats()
    print("pass 1: index_kind", st["index_kind"], "ms_index_build", repr(st["ms_index_build"]))
    assert e.partitions() == [0, len(TARGETS_NOX)]
    assert st["index_kind"] == 0
    assert first.shape == full.shape and (first == full).all()
    for n in (2, 3):
        again = srt(raw_hits(e, c, False))
        st_n = e.stats()
        print("pass", n, ": ms_index_build", repr(st_n["ms_index_build"]))
        assert again.shape == first.shape and (again == first).all()
        assert st_n["ms_index_build"] == st["ms_index_build"], (n, st_n["ms_index_build"], st["ms_index_build"])
