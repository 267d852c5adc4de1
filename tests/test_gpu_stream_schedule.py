"""The streamed step's schedule on the GPU: musc_reads_load_packed32(async) queues the upload on the pieces of
stream_plan, the pass that consumes it runs on the plan's tapered batches, the record buffer is kept from load to load,
and musc_hits_copy_compact / musc_hits_copy_packed to the host pack and copy chunk by chunk.  None of it may change a
tuple: everything is compared with the blocking load, with the literal oracle, and with the single-launch download to a
device buffer -- on the four paths the suite parametrises, with MUSC_BATCH_READS small enough that a few thousand reads
cross every edge of the plan (batches of 320, pieces of 128, a last batch of at most 64; download chunks of 320)."""
import os

import numpy as np
import pytest

from oracle import literal
from oracle import muscato_oracle as orc

pytestmark = pytest.mark.gpu

BATCH = 320
L = 100
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
KNOBS = ("MUSC_INDEX", "MUSC_MATCH", "MUSC_BATCH_READS", "MUSC_GRAPH", "MUSC_NO_SPEC", "MUSC_DEBUG_INDEX_BUDGET_MB")
PATHS = {"auto": {}, "dma": {"MUSC_MATCH": "dma"}, "classic": {"MUSC_INDEX": "classic"}, "lines": {"MUSC_INDEX": "lines"}}
# read counts at the plan's edges: below / at / above a wave-tile, a piece, a batch, two batches; ragged larger ones
COUNTS = [1, 63, 64, 65, 127, 128, 129, 256, 319, 320, 321, 640, 641, 1500, 3000]


def _targets(seed=17):
    rng = np.random.default_rng(seed)
    return [bytes(BASES[rng.integers(0, 4, int(n))]) for n in np.r_[rng.integers(150, 2500, 50), rng.integers(4000, 9000, 6)]]


TARGETS = _targets()
NB = sum(len(t) for t in TARGETS)


def _reads(seed, n):
    """n distinct reads of L bases, sorted: most of them mutated pieces of the targets, some random"""
    rng = np.random.default_rng(seed)
    tl = np.array([len(t) for t in TARGETS])
    out = set()
    while len(out) < n:
        if rng.random() < 0.15:
            out.add(bytes(BASES[rng.integers(0, 4, L)]))
            continue
        g = int(rng.integers(0, len(TARGETS)))
        p = int(rng.integers(0, tl[g] - L + 1))
        a = np.frombuffer(TARGETS[g][p:p + L], dtype=np.uint8).copy()
        sub = rng.random(L) < 0.03
        a[sub] = BASES[rng.integers(0, 4, size=int(sub.sum()))]
        out.add(bytes(a))
    return sorted(out)


READS = _reads(5, 3000)


def ocfg(**kw):
    c = dict(Windows=[0, 20], WindowWidth=15, PMatch=0.95, MinDinuc=0, MaxReadLength=L, MaxMatches=1000000, MMTol=1)
    c.update(kw)
    return orc.Config(**c)


def to_cfg(c):
    from muscato_amd import Config
    return Config(Windows=list(c.Windows), WindowWidth=c.WindowWidth, PMatch=c.PMatch, MinDinuc=c.MinDinuc,
                  MaxReadLength=c.MaxReadLength, MaxMatches=c.MaxMatches, MMTol=c.MMTol, MatchMode=c.MatchMode)


_ORACLE = {}


def oracle(reads, targets, c):
    """(every accepted tuple, best + MMTol), sorted; MaxMatches out of the way: the library keeps every tuple"""
    key = (hash(tuple(reads)), hash(tuple(targets)), c.PMatch, c.MMTol)
    if key not in _ORACLE:
        gbuf, goff = literal.concat(targets)
        rbuf, roff = literal.concat(reads)
        big = orc.Config(**dict(c.__dict__, MaxMatches=2 ** 31 - 1))
        full, _, _ = literal.match_arrays(rbuf, roff, gbuf, goff, literal.make_params(big, bloom_size=16_000_000, num_hash=8, nthreads=8))
        best = np.array(sorted(orc.best_filter(map(tuple, full.tolist()), c.MMTol)), dtype=np.uint32).reshape(-1, 4)
        _ORACLE[key] = (full, best)
    return _ORACLE[key]


def srt(a):
    from muscato_amd import sorted_hits
    return sorted_hits(a)


def same(got, exp):
    assert got.shape == exp.shape, "tuple count differs: %d vs %d" % (len(got), len(exp))
    assert (got == exp).all()


class Stream:
    """reads of L bases as the bare 2-bit stream, kept alive while the library borrows it"""

    def __init__(self, reads):
        from muscato_amd.api import concat, pack_2bit
        self.n = len(reads)
        if reads:
            buf, off = concat(reads)
            packed, mask = pack_2bit(buf, int(off[-1]))
            assert mask is None
        else:
            packed = np.zeros(0, np.uint8)
        self.packed = np.concatenate([packed, np.zeros(8, np.uint8)])

    def load(self, e, asyn):
        e.load_reads_packed32_ptr(self.packed.ctypes.data, 0, 0, L, self.n, async_upload=asyn)


@pytest.fixture(params=list(PATHS))
def engine(request):
    """-> make(extra_env): an Engine on the path of the parametrisation, MUSC_BATCH_READS read at its musc_init"""
    made = []

    def make(extra=None, batch=BATCH):
        from muscato_amd import Engine
        old = {k: os.environ.get(k) for k in KNOBS}
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(PATHS[request.param])
        os.environ["MUSC_BATCH_READS"] = str(batch)
        os.environ.update(extra or {})
        try:
            e = Engine(0)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        made.append(e)
        return e

    yield make
    for e in made:
        e.close()


def raw(e, c, apply_mmtol):
    n = e.match_device(to_cfg(c), apply_mmtol=apply_mmtol)
    out = np.zeros((n, 4), dtype=np.uint32)
    if n:
        e.hits_to(out.ctypes.data, n, False)
    return out


def test_counts_at_the_plans_edges(engine):
    """async load + match = blocking load + match = the oracle (every tuple, best + MMTol, the MaxMatches verdict),
    the streamed pass on exactly the plan's batches."""
    from muscato_amd.api import stream_plan
    e = engine()
    e.load_targets(TARGETS)
    c = ocfg()
    for n in COUNTS:
        reads = READS[:n]
        full, best = oracle(reads, TARGETS, c)
        s = Stream(reads)
        plan = stream_plan(n, L, BATCH)
        for asyn in (True, False):
            for apply_mmtol, exp in ((False, full), (True, best)):
                s.load(e, asyn)
                same(srt(raw(e, c, apply_mmtol)), exp)
                st = e.stats()
                assert st["n_overflow_blocks"] == 0, (n, asyn)
                if asyn:
                    assert st["n_batches"] == len(plan["batch_ends"]) == plan["planned_batches"], (n, st["n_batches"])
                else:
                    assert st["n_batches"] == (n + BATCH - 1) // BATCH, (n, st["n_batches"])


def test_record_buffer_reuse_regrow_and_the_sized_state(engine):
    """Twice in a row on one engine (the record buffer reused), a smaller and a larger read set (capacity reuse and
    regrow), reads of another loader in between; then async load -> match -> match again: the streamed pass leaves the
    context unsized, the next pass over the same reads sizes itself on uniform batches and the one after replays it."""
    from muscato_amd.api import stream_plan
    e = engine()
    e.load_targets(TARGETS)
    c = ocfg()
    for n in (1500, 1500, 321, 3000, 0, 1, 3000):
        s = Stream(READS[:n])
        s.load(e, True)
        got = srt(raw(e, c, True))
        if n:
            same(got, oracle(READS[:n], TARGETS, c)[1])
        else:
            assert len(got) == 0
    e.load_reads(READS[:100])  # (the general loader replaces the buffer)
    same(srt(raw(e, c, True)), oracle(READS[:100], TARGETS, c)[1])
    n = 2000
    s = Stream(READS[:n])
    exp = oracle(READS[:n], TARGETS, c)[1]
    s.load(e, True)
    first = raw(e, c, True)
    assert e.stats()["n_batches"] == len(stream_plan(n, L, BATCH)["batch_ends"])
    uniform = (n + BATCH - 1) // BATCH
    second = raw(e, c, True)
    assert e.stats()["n_batches"] == uniform, "the pass after a streamed one did not size itself on uniform batches"
    third = raw(e, c, True)
    assert e.stats()["n_batches"] == uniform
    for got in (first, second, third):
        same(srt(got), exp)
    # an upload nobody matches is waited for when the next one replaces it
    s.load(e, True)
    s2 = Stream(READS[:700])
    s2.load(e, True)
    same(srt(raw(e, c, True)), oracle(READS[:700], TARGETS, c)[1])


@pytest.mark.parametrize("max_matches", [1, 25, 10 ** 6])
def test_max_matches_verdict(engine, max_matches):
    """Screening (10^6), the trip into the exact re-run (25: the threshold per workgroup and batch falls below two)
    and MaxMatches 1: the streamed pass's tuples and verdict are the blocking run's."""
    e = engine()
    e.load_targets(TARGETS)
    c = ocfg(MaxMatches=max_matches)
    n = 3000
    s = Stream(READS[:n])
    full, best = oracle(READS[:n], TARGETS, c)
    got = {}
    for asyn in (False, True):
        s.load(e, asyn)
        h = raw(e, c, True)
        same(srt(h), best)
        got[asyn] = (e.stats()["n_overflow_blocks"], len(e.overflow_probes()))
        s.load(e, asyn)
        same(srt(raw(e, c, False)), full)
    assert got[True] == got[False], got
    if max_matches == 10 ** 6:
        assert got[True] == (0, 0)
    if max_matches == 1:
        assert got[True][0] >= 1  # (two reads of one target segment share a window key)


def test_partitioned_database(engine):
    """The upload feeds the first partition's pass (on the plan's batches), the later partitions find the reads resident."""
    e = engine()
    e.load_targets(TARGETS)
    e.set_partition_bases((NB + 2) // 3)
    c = ocfg()
    n = 1500
    s = Stream(READS[:n])
    full, best = oracle(READS[:n], TARGETS, c)
    for rep in range(2):
        s.load(e, True)
        same(srt(raw(e, c, True)), best)
        assert len(e.partitions()) > 3
    s.load(e, True)
    same(srt(raw(e, c, False)), full)


def _compact(e, n, nr, on_device, bits):
    """musc_hits_copy_compact to host arrays, or to a device buffer copied back"""
    import torch
    if on_device:
        w = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
        k = torch.zeros(max(nr, 1), dtype=torch.uint8, device="cuda")
        e.hits_to_compact(w.data_ptr(), n, k.data_ptr(), nr, True, bits)
        torch.cuda.synchronize()
        return w.cpu().numpy().view(np.uint32)[:n], k.cpu().numpy()[:nr]
    w = np.full(max(n, 1), 0xFFFFFFFF, np.uint32)
    k = np.full(max(nr, 1), 0xFF, np.uint8)
    e.hits_to_compact(w.ctypes.data, n, k.ctypes.data, nr, False, bits)
    return w[:n], k[:nr]


def test_compact_and_packed_downloads_host_equals_device(engine):
    """0 tuples, 1 tuple, a list that is several chunks and no multiple of one, and a read with 256 tuples (the verdict
    "more than 255" on both ways); the 8-byte packed form likewise."""
    import torch
    from muscato_amd import MuscatoError
    e = engine()
    e.load_targets(TARGETS)
    bits = (6, 14, 4)
    rng = np.random.default_rng(9)
    cases = {"none": ([bytes(BASES[rng.integers(0, 4, L)]) for _ in range(5)], ocfg(PMatch=1.0)),
             "one": ([TARGETS[3][7:7 + L]], ocfg(PMatch=1.0)),
             "many": (READS[:3000], ocfg())}
    for name, (reads, c) in cases.items():
        reads = sorted(reads)
        Stream(reads).load(e, False)
        hits = raw(e, c, False if name == "many" else True)
        n, nr = len(hits), len(reads)
        assert {"none": n == 0, "one": n == 1, "many": n > 3 * BATCH and n % BATCH != 0}[name], (name, n)
        hw, hk = _compact(e, n, nr, False, bits)
        dw, dk = _compact(e, n, nr, True, bits)
        assert (hw == dw).all() and (hk == dk).all(), name
        assert int(hk.sum()) == n
        dec = np.stack([np.repeat(np.arange(nr, dtype=np.uint32), hk), hw >> 18, (hw >> 4) & 0x3FFF, hw & 15], axis=1).astype(np.uint32)
        assert (dec == hits).all(), name
        if n:
            pbits = (12, 6, 14, 4)
            h64 = np.zeros(n, np.uint64)
            e.hits_to_packed(h64.ctypes.data, n, False, pbits, 5)
            d64 = torch.zeros(n, dtype=torch.int64, device="cuda")
            e.hits_to_packed(d64.data_ptr(), n, True, pbits, 5)
            torch.cuda.synchronize()
            assert (h64 == d64.cpu().numpy().view(np.uint64)).all(), name
            assert ((h64 >> np.uint64(24)) == hits[:, 0].astype(np.uint64) + np.uint64(5)).all()
            with pytest.raises(MuscatoError, match="does not fit"):
                e.hits_to_compact(hw.ctypes.data, n, hk.ctypes.data, nr, False, (2, 14, 4) if name == "many" else (1, 2, 1))
    # a read with 256 tuples: one segment 256 times in the database
    seg = bytes(BASES[rng.integers(0, 4, L)])
    e.load_targets([seg + bytes(BASES[rng.integers(0, 4, 20)]) for _ in range(256)])
    reads = sorted([seg, bytes(BASES[rng.integers(0, 4, L)])])
    Stream(reads).load(e, True)
    hits = raw(e, ocfg(PMatch=1.0), True)
    assert len(hits) == 256
    for on_device in (False, True):
        with pytest.raises(MuscatoError, match="more than 255"):
            _compact(e, 256, 2, on_device, (9, 8, 4))
