"""Every read and database loader, byte for byte against its input.

The readback: musc_results_order on a hand-fed host list, then musc_results_text, renders a tuple's read from the 2-bit
records (rd / rdm, with the length and the READ_HAS_X word) and target[pos : pos + len(read)] from the database planes
(db2 / dbm2).  k_results_render is held to the oracle by tests/test_gpu_results.py; here it is the window through which
what the loaders left on the device is compared with what went in -- also the reads that match nothing and the target
bases no read lands on, which a match never looks at.  Inputs and expected text: tests/loader_cases.py (their coverage
of start phases, record strides and X placements is asserted in tests/test_loader_cases.py).  Every comparison is exact
equality of bytes or of tuple arrays."""
import random

import numpy as np
import pytest

from muscato_amd import Config, Engine, MuscatoError, sorted_hits
from oracle import muscato_oracle as orc

import loader_cases as lc
from cases import check_groups, mutate, rand_seq

pytestmark = pytest.mark.gpu

PROBE_TARGETS = [b"ACGT" * 8]
PROBE_RESTS = [b"probe\t32"]
PROBE_CFG = Config(Windows=[0], WindowWidth=8, PMatch=1.0, MaxReadLength=1000)


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


def probe_db(e):
    e.load_targets(PROBE_TARGETS)
    e.set_gene_text(PROBE_RESTS)


def assert_reads_resident(e, reads):
    """The loaded reads, rendered one line each, are `reads`."""
    assert e.n_reads == len(reads)
    hits = [(r, 0, 0, 0) for r in range(len(reads))]
    exp = b"".join(lc.expected_lines(reads, PROBE_TARGETS, PROBE_RESTS, hits))
    nl, nb = e.results_order(np.array(hits, dtype=np.uint32).reshape(-1, 4))
    assert nl == len(reads)
    got = e.results_text()
    if got != exp:  # name the first read that differs: the whole text is too long to read
        gl, el = got.split(b"\n"), exp.split(b"\n")
        bad = next((i for i, (a, b) in enumerate(zip(gl, el)) if a != b), min(len(gl), len(el)))
        raise AssertionError("read %d of %d: got %r, expected %r" % (bad, len(reads), gl[bad:bad + 1], el[bad:bad + 1]))
    assert nb == len(exp)


class Packed:
    """A read or target list in the ABI's packed form (the reference packer's), with the arrays kept alive."""

    def __init__(self, seqs, garbage=False):
        self.n = len(seqs)
        self.off = lc.offsets_of(seqs)
        self.lens = np.array([len(s) for s in seqs], dtype=np.uint32)
        self.b2, self.bm, self.nx = lc.ref_pack(b"".join(seqs), random.Random(11) if garbage else None)


# ---------------------------------------------------------------- ragged reads

@pytest.mark.parametrize("with_x", [False, True], ids=["plain", "x"])
@pytest.mark.parametrize("maxlen", lc.RAGGED_MAXLENS)
def test_ragged_reads_ascii(eng, maxlen, with_x):
    """k_pack_reads<false>: host ASCII, and ASCII already on the device."""
    import torch
    reads = lc.ragged_reads(maxlen, with_x)
    probe_db(eng)
    eng.load_reads(reads)
    assert_reads_resident(eng, reads)
    buf = np.frombuffer(b"".join(reads) + b"\0" * 8, dtype=np.uint8).copy()
    d_buf = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(lc.offsets_of(reads).view(np.int64)).cuda()
    torch.cuda.synchronize()
    eng.load_reads(reads[:3])  # (so that the device load does not find the records it is to make)
    eng.load_reads_device(d_buf.data_ptr(), d_off.data_ptr(), len(reads))
    assert_reads_resident(eng, reads)


@pytest.mark.parametrize("with_x", [False, True], ids=["plain", "x"])
@pytest.mark.parametrize("maxlen", lc.RAGGED_MAXLENS)
def test_ragged_reads_packed(eng, maxlen, with_x):
    """k_pack_reads<true> behind 64-bit offsets and behind 32-bit lengths (k_widen_u32 + the scan), without a mask, with
    an all-zero mask (the plane is made and released), with a mask, and with garbage codes under the mask's bits."""
    reads = lc.ragged_reads(maxlen, with_x)
    probe_db(eng)
    forms = [(Packed(reads), True), (Packed(reads, garbage=True), True)] if with_x else [(Packed(reads), False), (Packed(reads), True)]
    for pk, use_mask in forms:
        assert (pk.nx > 0) == with_x
        mp = pk.bm.ctypes.data if use_mask else 0
        eng.load_reads(reads[:3])
        eng.load_reads_packed_ptr(pk.b2.ctypes.data, mp, pk.off.ctypes.data, pk.n)
        assert_reads_resident(eng, reads)
        eng.load_reads(reads[:3])
        eng.load_reads_packed32_ptr(pk.b2.ctypes.data, mp, pk.lens.ctypes.data, 0, pk.n)
        assert_reads_resident(eng, reads)


# ---------------------------------------------------------------- reads of one length

@pytest.mark.parametrize("L", lc.FIXED_LENS)
def test_fixed_length_reads(eng, L):
    """k_pack_reads_fixed at every bit phase its 64-bit extraction starts at, and the same stream with a mask and no
    lengths: offsets from k_iota_mul, records from k_pack_reads<true>."""
    probe_db(eng)
    reads = lc.fixed_reads(L, False)
    pk = Packed(reads)
    assert pk.nx == 0
    eng.load_reads_packed32_ptr(pk.b2.ctypes.data, 0, 0, L, pk.n)
    assert_reads_resident(eng, reads)
    xreads = lc.fixed_reads(L, True)
    for garbage in (False, True):
        xp = Packed(xreads, garbage)
        assert xp.nx > 0
        eng.load_reads_packed32_ptr(xp.b2.ctypes.data, xp.bm.ctypes.data, 0, L, xp.n)
        assert_reads_resident(eng, xreads)
    # an all-zero mask: the same branch, and the plane it made is released
    eng.load_reads_packed32_ptr(pk.b2.ctypes.data, pk.bm.ctypes.data, 0, L, pk.n)
    assert_reads_resident(eng, reads)


@pytest.mark.parametrize("batch", ["320", "257"])
def test_fixed_length_reads_streamed(batch, monkeypatch):
    """The streamed upload: pieces on the copy stream, records made batch by batch by the pass that consumes them.  The
    readback follows that pass.  L = 250 first, then 37: the second load reuses the staging and record buffers of the
    first, which are larger than it needs."""
    monkeypatch.setenv("MUSC_BATCH_READS", batch)  # read at musc_init
    monkeypatch.delenv("MUSC_INDEX", raising=False)
    with Engine(0) as e:
        probe_db(e)
        for L in (250, 37) + tuple(x for x in lc.FIXED_LENS if x not in (250, 37)):
            reads = lc.fixed_reads(L, False)
            pk = Packed(reads)
            e.load_reads_packed32_ptr(pk.b2.ctypes.data, 0, 0, L, pk.n, async_upload=True)
            with pytest.raises(MuscatoError, match="streamed read load"):
                e.results_order(np.zeros((1, 4), dtype=np.uint32))
            got = e.match(PROBE_CFG, apply_mmtol=False)
            exp = np.array(sorted(orc.match_direct(reads, PROBE_TARGETS, orc.Config(Windows=[0], WindowWidth=8, PMatch=1.0, MaxReadLength=1000))),
                           dtype=np.uint32).reshape(-1, 4)
            assert sorted_hits(got).tolist() == exp.tolist()
            st = e.stats()
            assert st["n_reads"] == len(reads) and st["n_batches"] > 1
            assert_reads_resident(e, reads)


# ---------------------------------------------------------------- read prep

def check_prep(eng, raw):
    probe_db(eng)
    order, ustart = eng.sort_unique_reads(raw)
    uniq = check_groups(raw, order, ustart)
    assert uniq == sorted(set(raw))
    assert_reads_resident(eng, uniq)


@pytest.mark.parametrize("with_x", [False, True], ids=["plain", "x"])
@pytest.mark.parametrize("maxlen", lc.RAGGED_MAXLENS)
def test_read_prep_records(eng, maxlen, with_x):
    """k_prep_pack: the records musc_reads_sort_unique leaves are sorted(set(reads)), base for base."""
    check_prep(eng, lc.with_duplicates(lc.ragged_reads(maxlen, with_x), maxlen))


def test_read_prep_prefixes_of_a_long_read(eng):
    """48 key words: every key-word boundary is crossed by a prefix, its extensions and its near-twins."""
    check_prep(eng, list(lc.prefix_reads()))


# ---------------------------------------------------------------- the database

PROBE_READ = lc.rand_bases(random.Random(300), 300)  # longer than every target: a span is the rest of its target


def assert_targets_resident(e, targets):
    rests = lc.target_rests(targets)
    e.set_gene_text(rests)
    e.load_reads([PROBE_READ])
    hits = lc.target_tuples(targets)
    exp = lc.expected_lines([PROBE_READ], targets, rests, hits)
    nl, nb = e.results_order(np.array(hits, dtype=np.uint32))
    got = e.results_text().splitlines(True)
    assert nl == len(got) == len(exp) == len(targets) + 5
    assert sorted(got) == sorted(exp)
    assert nb == sum(len(x) for x in exp)


@pytest.mark.parametrize("with_x", [False, True], ids=["plain", "x"])
def test_database_ascii(eng, with_x):
    """k_pack_db_ascii from the host and from the device; without X the mask plane is released."""
    import torch
    targets = lc.target_set(with_x)
    eng.load_targets(targets)
    assert_targets_resident(eng, targets)
    buf = np.frombuffer(b"".join(targets) + b"\0" * 8, dtype=np.uint8).copy()
    d_buf = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(lc.offsets_of(targets).view(np.int64)).cuda()
    torch.cuda.synchronize()
    eng.load_targets(PROBE_TARGETS)
    eng.load_targets_device(d_buf.data_ptr(), d_off.data_ptr(), len(targets))
    assert_targets_resident(eng, targets)


@pytest.mark.parametrize("form", ["plain", "plain-zero-mask", "x", "x-garbage"])
def test_database_packed(eng, form):
    """k_pack_db_packed: Engine.load_targets_packed (pack_2bit's stream), and the reference packer's stream through the
    ABI -- once with random non-zero codes under the mask's bits, which the header says are ignored."""
    targets = lc.target_set(form.startswith("x"))
    eng.load_targets(PROBE_TARGETS)
    if form in ("plain", "x"):
        eng.load_targets_packed(targets)
        assert_targets_resident(eng, targets)
        eng.load_targets(PROBE_TARGETS)
    pk = Packed(targets, garbage=form == "x-garbage")
    assert (pk.nx > 0) == form.startswith("x")
    mp = None if form == "plain" else pk.bm.ctypes.data
    eng._check(eng._lib.musc_db_load_packed(eng._h, pk.b2.ctypes.data, mp, pk.off.ctypes.data, pk.n), "musc_db_load_packed")
    eng.n_targets = pk.n
    assert_targets_resident(eng, targets)


# ---------------------------------------------------------------- the same tuples, whichever way the bases came in

@pytest.fixture(scope="module")
def workload():
    """60 targets of 700 bases, 3000 reads of L bases cut from them with 2 % substitutions, the same reads with about 1 %
    X, and the oracle's tuples of both -- made once per L."""
    made = {}

    def get(L):
        if L not in made:
            rng = random.Random(1000 + L)
            targets = [rand_seq(rng, 700, b"ACGT") for _ in range(60)]
            rs = set()
            while len(rs) < 3000:
                t = rng.choice(targets)
                p = rng.randint(0, len(t) - L)
                rs.add(mutate(rng, t[p:p + L], 0.02, b"ACGT"))
            reads = sorted(rs)
            xreads = [bytes(ord("X") if rng.random() < 0.01 else c for c in r) for r in reads]
            ocfg = orc.Config(Windows=[0, 11], WindowWidth=10, PMatch=0.95, MinDinuc=2, MaxReadLength=L, MaxMatches=100000, MMTol=1)
            as_arr = lambda hits: np.array(sorted(hits), dtype=np.uint32).reshape(-1, 4)
            made[L] = (targets, reads, xreads, ocfg, as_arr(orc.match_direct(reads, targets, ocfg)), as_arr(orc.match_direct(xreads, targets, ocfg)))
        return made[L]
    return get


@pytest.mark.parametrize("L", [37, 101])
@pytest.mark.parametrize("index", ["auto", "classic"])
def test_same_tuples_through_every_fixed_length_loader(index, L, workload, monkeypatch):
    targets, reads, xreads, ocfg, exp, xexp = workload(L)
    assert len(exp) > 2000 and len(xexp) > 500 and sum(1 for r in xreads if b"X" in r) > 300
    cfg = Config(Windows=list(ocfg.Windows), WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                 MaxReadLength=ocfg.MaxReadLength, MaxMatches=ocfg.MaxMatches, MMTol=ocfg.MMTol)
    monkeypatch.delenv("MUSC_MATCH", raising=False)
    monkeypatch.delenv("MUSC_INDEX", raising=False)
    if index == "classic":
        monkeypatch.setenv("MUSC_INDEX", "classic")
    monkeypatch.setenv("MUSC_BATCH_READS", "320")  # several batches, and several pieces of the streamed upload
    pk, xp = Packed(reads), Packed(xreads)
    assert pk.nx == 0 and xp.nx > 0

    def same(e, want, n):
        got = sorted_hits(e.match(cfg, apply_mmtol=False))
        assert got.shape == want.shape and (got == want).all()
        assert e.stats()["n_reads"] == n

    with Engine(0) as e:
        e.load_targets(targets)
        e.load_reads(reads)
        same(e, exp, len(reads))
        if index == "classic":
            assert e.stats()["index_kind"] in (0, 3)
        e.load_reads(reads[:5])
        e.load_reads_packed32_ptr(pk.b2.ctypes.data, 0, 0, L, pk.n)
        same(e, exp, len(reads))
        e.load_reads(reads[:5])
        e.load_reads_packed32_ptr(pk.b2.ctypes.data, 0, 0, L, pk.n, async_upload=True)
        same(e, exp, len(reads))
        same(e, exp, len(reads))  # the repeat pass finds the records resident
        e.load_reads_packed32_ptr(xp.b2.ctypes.data, xp.bm.ctypes.data, 0, L, xp.n)
        same(e, xexp, len(xreads))


# ---------------------------------------------------------------- refused loads

def small_case():
    rng = random.Random(21)
    targets = [rand_seq(rng, 300, b"ACGT") for _ in range(20)]
    reads = sorted({mutate(rng, t[p:p + 60], 0.02, b"ACGT") for t in targets for p in (0, 57, 240)})
    return orc.Config(Windows=[0, 10], WindowWidth=12, PMatch=0.95, MinDinuc=2, MaxReadLength=60, MMTol=1), reads, targets


def refused(call):
    with pytest.raises(MuscatoError, match=r"failed \(2\)"):
        call()


def test_refused_loads_leave_nothing_stale(eng):
    """A load that the library refuses from the offsets or the lengths alone (offsets[0] != 0, a read of more than 65 535
    bases, a database of no targets or of 2^36 bases) leaves no reads -- or no database -- behind: the next match raises or returns nothing, never the tuples of
    what was loaded before."""
    ocfg, reads, targets = small_case()
    cfg = Config(Windows=list(ocfg.Windows), WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                 MaxReadLength=ocfg.MaxReadLength, MMTol=ocfg.MMTol)
    exp = np.array(sorted(orc.match_direct(reads, targets, ocfg)), dtype=np.uint32).reshape(-1, 4)
    assert len(exp) > 40

    def good():
        got = sorted_hits(eng.match(cfg, apply_mmtol=False))
        assert got.shape == exp.shape and (got == exp).all()

    def nothing():
        try:
            got = eng.match(cfg, apply_mmtol=False)
        except MuscatoError:
            return
        assert len(got) == 0

    buf = np.frombuffer(b"".join(reads) + b"\0" * 8, dtype=np.uint8).copy()
    off1 = lc.offsets_of(reads)
    off1[0] = 1  # (the first read has 60 bases: the offsets still do not decrease)
    long_buf = np.frombuffer(b"ACGT" * 16384 + b"\0" * 8, dtype=np.uint8).copy()
    long_off = np.array([0, 65536], dtype=np.uint64)
    long_b2 = np.zeros(65536 // 4 + 16, dtype=np.uint8)
    refusals = [
        lambda: eng.load_reads_arrays(buf, off1),
        lambda: eng.load_reads_arrays(long_buf, long_off),
        lambda: eng.load_reads_packed32_ptr(long_b2.ctypes.data, 0, 0, 65536, 1),
        lambda: eng.sort_unique_reads_arrays(buf.ctypes.data, off1.ctypes.data, len(reads), False),
        lambda: eng.sort_unique_reads_arrays(long_buf.ctypes.data, long_off.ctypes.data, 1, False),
    ]
    eng.load_targets(targets)
    for call in refusals:
        eng.load_reads(reads)
        good()
        refused(call)
        nothing()
    eng.load_reads(reads)
    good()
    # the database
    tbuf = np.frombuffer(b"".join(targets) + b"\0" * 8, dtype=np.uint8).copy()
    toff1 = lc.offsets_of(targets)
    toff1[0] = 1
    refused(lambda: eng.load_targets_arrays(tbuf, toff1))
    nothing()
    # every early exit of the database's shape, through both loaders that reach it: no target at all, offsets that do not
    # start at 0, and more than 2^36 bases (refused from the offsets alone: the 16 bytes are never read)
    pk = Packed(targets)
    no_off = np.zeros(1, dtype=np.uint64)
    huge_off = np.array([0, 1 << 36], dtype=np.uint64)
    dummy = np.zeros(16, dtype=np.uint8)

    def load_packed(off, nseq):
        eng._check(eng._lib.musc_db_load_packed(eng._h, pk.b2.ctypes.data, None, off.ctypes.data, nseq), "musc_db_load_packed")

    for call in (lambda: eng.load_targets_arrays(tbuf, no_off),
                 lambda: load_packed(no_off, 0),
                 lambda: eng.load_targets_arrays(dummy, huge_off),
                 lambda: load_packed(toff1, len(targets))):
        eng.load_targets(targets)
        good()
        refused(call)
        nothing()
    eng.load_targets(targets)
    good()


def test_longest_read_the_record_takes(eng):
    """One read of 65 535 bases, the most the 16-bit length of a record holds, through the ASCII loader and through
    the read prep: accepted and read back whole, its span clipped at the end of a 40-base target."""
    rng = random.Random(65535)
    b = bytearray(lc.rand_bases(rng, 65535))
    for p in (0, 15, 16, 4095, 32768, 65534):
        b[p] = ord("X")
    read = bytes(b)
    target = lc.rand_bases(rng, 40)
    rests = [b"short\t40"]

    def check():
        eng.set_gene_text(rests)
        exp = lc.expected_lines([read], [target], rests, [(0, 0, 0, 0)])[0]
        nl, nb = eng.results_order(np.array([(0, 0, 0, 0)], dtype=np.uint32))
        got = eng.results_text()
        assert (nl, nb, len(got)) == (1, len(exp), len(exp)) and len(exp) == 65535 + 1 + 40 + len(b"\t0\t0\tshort\t40\n")
        assert got == exp, "the 65 535-base read came back changed"

    eng.load_targets([target])
    eng.load_reads([read])
    check()
    eng.load_reads([b"ACGT"])
    order, ustart = eng.sort_unique_reads([read, read])
    assert order.tolist() == [0, 1] and ustart.tolist() == [0, 2] and eng.n_reads == 1
    check()
