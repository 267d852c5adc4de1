"""Target preparation on the GPU: musc_targets_prep, musc_targets_prep_text, musc_targets_prep_load,
musc_targets_prep_free and musc_sz_frame against tests/targets_prep_cases.py, whose cases and model
tests/test_targets_prep_cases.py holds to the oracle without a GPU.

Both texts and the info struct of every case, with and without reverse complements, from the text on the host and on
the device at sixteen address offsets between bytes that would change the answer if they were read; ranges of a text
into device memory at sixteen alignments between guard bytes; the refusals and what a context holds afterwards; the
database that load_db_prepared makes, base for base through the results renderer (tests/loader_cases.py) and by the
tuples of an oracle case on the picked and on the classic index; the framed writer against tests/sz_cases.py's and the
oracle's decoder.  Every comparison is exact."""
import ctypes
import functools
import random

import numpy as np
import pytest

from muscato_amd import Config, Engine, MuscatoError, sorted_hits
from oracle import muscato_oracle as orc

import loader_cases as lc
import sz_cases as sc
import targets_prep_cases as tp
from cases import make_case

pytestmark = pytest.mark.gpu

GUARD = 0xA5
AROUND = b"\n>\t"  # around a text on the device: bytes that would change the answer if they were read
PROBE_LEN = 1000
PROBE_READ = b"ACGT" * (PROBE_LEN // 4)
CASES = tp.all_cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def expected(name, rev):
    c = BY_NAME[name]
    m = tp.model(c.text, c.fasta, rev)
    return (m,) + tp.texts_of(m)


def on_device(torch, text, k):
    """`text` in device memory at address offset k (mod 16), AROUND on both sides: the tensor and the pointer."""
    h = np.frombuffer(AROUND * ((len(text) + 96) // len(AROUND) + 1), dtype=np.uint8)[:len(text) + 64].copy()
    h[16 + k:16 + k + len(text)] = np.frombuffer(text, dtype=np.uint8)
    d = torch.from_numpy(h).cuda()
    torch.cuda.synchronize()
    assert d.data_ptr() % 16 == 0
    return d, d.data_ptr() + 16 + k


def check_prepared(e, name, rev, info):
    c = BY_NAME[name]
    m, seqs, ids = expected(name, rev)
    assert (info.n_lines, info.n_records, info.n_targets, info.n_dropped, info.stop_line, info.n_subx, info.n_seq_bytes, info.n_id_bytes) == \
        (m.n_lines, len(m.seqs) // (2 if rev else 1), len(m.seqs), m.n_dropped, m.stop_line, m.n_subx, len(seqs), len(ids))
    assert info.ms >= 0 and (info.ms > 0 or not c.text)
    got = e.prepared_text(0)
    if got != seqs:
        bad = next((i for i, (a, b) in enumerate(zip(got, seqs)) if a != b), min(len(got), len(seqs)))
        raise AssertionError("sequence text: byte %d of %d / %d: got %r, expected %r" % (bad, len(got), len(seqs), got[bad:bad + 24], seqs[bad:bad + 24]))
    got = e.prepared_text(1)
    if got != ids:
        bad = next((i for i, (a, b) in enumerate(zip(got, ids)) if a != b), min(len(got), len(ids)))
        raise AssertionError("id text: byte %d of %d / %d: got %r, expected %r" % (bad, len(got), len(ids), got[bad:bad + 40], ids[bad:bad + 40]))


def prep(e, name, rev, data, dev):
    """prep_targets of a case: checked against the model, or refused with 14 and the model's line."""
    c = BY_NAME[name]
    m = expected(name, rev)[0]
    if m.refused is None:
        check_prepared(e, name, rev, e.prep_targets(data, c.fasta, rev, on_device=dev))
        return
    with pytest.raises(MuscatoError) as ei:
        e.prep_targets(data, c.fasta, rev, on_device=dev)
    assert str(ei.value) == "musc_targets_prep failed (14): musc_targets_prep: empty line in FASTA input (line %d)" % m.refused
    with pytest.raises(MuscatoError, match=r"failed \(2\)"):
        e.prepared_text(0, 0, 0)


# ---------------------------------------------------------------- both texts and the info struct

@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_prep_host(eng, name, rev):
    prep(eng, name, rev, BY_NAME[name].text, False)


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_prep_device_sixteen_offsets(eng, torch, name, rev):
    text = BY_NAME[name].text
    for k in range(16):
        d, ptr = on_device(torch, text, k)
        prep(eng, name, rev, (ptr, len(text)), True)


# ---------------------------------------------------------------- prepared_text

def raw_text(e, which, off, n, dst, dev):
    rc = e._lib.musc_targets_prep_text(e._h, which, off, n, dst, 1 if dev else 0)
    return rc, e._lib.musc_last_error(e._h).decode()


def test_prepared_text_ranges(eng, torch):
    name = "fa_3_tiles"
    eng.prep_targets(BY_NAME[name].text, True, True)
    _, seqs, ids = expected(name, True)
    for which, text in ((0, seqs), (1, ids)):
        n = len(text)
        for off, nb in ((0, 0), (0, n), (0, 1), (1, n - 1), (n, 0), (n - 1, 1), (7, min(4096, n - 7)), (n // 3 | 1, n // 2), (n // 2, n - n // 2)):
            assert eng.prepared_text(which, off, nb) == text[off:off + nb]
        assert eng.prepared_text(which, 5) == text[5:]
        # refused ranges
        for off, nb in ((n + 1, 0), (n, 1), (0, n + 1), (1, n), (2 ** 64 - 1, 2)):
            rc, msg = raw_text(eng, which, off, nb, np.zeros(8, dtype=np.uint8).ctypes.data, False)
            assert rc == 2 and "beyond the text" in msg
    assert raw_text(eng, 2, 0, 0, None, False)[0] == 2 and raw_text(eng, -1, 0, 0, None, False)[0] == 2
    assert raw_text(eng, 0, 0, 4, None, False)[0] == 2
    # device destinations at sixteen alignments between guards
    buf = torch.empty(5000 + 64, dtype=torch.uint8, device="cuda")
    for k in range(16):
        off, nb = 3 + 5 * k, 4990 + k
        buf.fill_(GUARD)
        torch.cuda.synchronize()
        rc, msg = raw_text(eng, 0, off, nb, buf.data_ptr() + 16 + k, True)
        assert rc == 0, msg
        got = buf.cpu().numpy()
        assert got[16 + k:16 + k + nb].tobytes() == seqs[off:off + nb], "offset %d" % k
        assert (got[:16 + k] == GUARD).all() and (got[16 + k + nb:] == GUARD).all(), "guard bytes, offset %d" % k


# ---------------------------------------------------------------- refusals and state

def test_refused_calls_and_what_stays(eng):
    good = b">a\nACGT\n>b\nGGNA\n"
    lib, h = eng._lib, eng._h
    src = np.frombuffer(good, dtype=np.uint8)
    for fasta, rev in ((2, 0), (-1, 0), (0, 2), (1, -1)):
        eng.prep_targets(good, True, False)
        assert lib.musc_targets_prep(h, src.ctypes.data, len(src), 0, fasta, rev, None) == 2
        with pytest.raises(MuscatoError, match=r"failed \(2\): musc_targets_prep_text: no prepared text"):  # a failed call clears an earlier result
            eng.prepared_text(0, 0, 1)
    eng.prep_targets(good, True, False)
    assert lib.musc_targets_prep(h, None, 5, 0, 1, 0, None) == 2
    assert raw_text(eng, 0, 0, 0, None, False)[0] == 2
    assert lib.musc_targets_prep(h, src.ctypes.data, len(src), 0, 1, 1, None) == 0  # no info asked for
    assert eng.prepared_text(0, 0, 10) == b"ACGT\nACGT\n"
    # 14 with the line number; nothing stays
    with pytest.raises(MuscatoError) as ei:
        eng.prep_targets(b">a\r\nAC\r\n\r\nGG\n\n", True, True)
    assert str(ei.value) == "musc_targets_prep failed (14): musc_targets_prep: empty line in FASTA input (line 2)"
    with pytest.raises(MuscatoError, match=r"failed \(2\)"):
        eng.prepared_text(1, 0, 0)
    with pytest.raises(MuscatoError, match=r"failed \(2\): musc_targets_prep_load: no prepared text"):
        eng.load_db_prepared()
    # the same bytes are a stop line in the text format
    info = eng.prep_targets(b"a\tAC\r\n\r\nb\tGG\n", False, True)
    assert (info.stop_line, info.n_records, info.n_targets) == (1, 1, 2) and eng.prepared_text(0) == b"AC\nGT\n"
    assert eng.prepared_text(1) == b"00000000000\ta\t2\n00000000001\ta_r\t2\n"
    eng.free_prepared()
    with pytest.raises(MuscatoError, match=r"no prepared text"):
        eng.prepared_text(0, 0, 0)
    eng.free_prepared()  # (nothing to free: fine)
    # the empty input: two empty texts, and no database in them
    info = eng.prep_targets(b"", True, True)
    assert (info.n_lines, info.n_targets, info.n_seq_bytes, info.n_id_bytes, info.stop_line) == (0, 0, 0, 0, tp.NO_STOP)
    assert eng.prepared_text(0) == b"" and eng.prepared_text(1) == b""
    with pytest.raises(MuscatoError, match=r"failed \(2\): database has no sequences"):
        eng.load_db_prepared()


def test_a_prep_leaves_the_other_stages_valid():
    """A prep between a pass and results_text: the tuples, the order and the text are those of a run without it."""
    ocfg, reads, targets = make_case(2)
    cfg = Config(Windows=ocfg.Windows, WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                 MaxReadLength=ocfg.MaxReadLength, MaxMatches=ocfg.MaxMatches, MMTol=ocfg.MMTol, MatchMode=ocfg.MatchMode)
    other = BY_NAME["fa_3_tiles"].text
    with Engine(0) as e:
        def run(with_prep):
            e.load_targets(targets)
            e.load_reads(reads)
            e.set_gene_text(lc.target_rests(targets))
            e.set_read_text([b"1\tr%d" % i for i in range(len(reads))])
            n = e.match_device(cfg)
            if with_prep:
                e.prep_targets(other, True, True)
            nl, nb = e.results_order()
            if with_prep:
                e.prep_targets(other[:5000], True, False)
            text = e.results_text()
            if with_prep:
                e.free_prepared()
            return n, nl, nb, text, sorted_hits(e.hits()).tolist()
        plain = run(False)
        assert plain[0] and plain[1] and plain == run(True)
        # ...and a load or a pass leaves the prepared texts alone
        e.prep_targets(other, True, True)
        e.load_targets(targets)
        e.load_reads(reads)
        e.match_device(cfg)
        assert (e.prepared_text(0), e.prepared_text(1)) == expected("fa_3_tiles", True)[1:]


# ---------------------------------------------------------------- load_db_prepared

LOADABLE = [(c.name, rev) for c in CASES for rev in (False, True)
            if expected(c.name, rev)[0].refused is None and expected(c.name, rev)[0].seqs and tp.acgtx_only(expected(c.name, rev)[0])]


@pytest.mark.parametrize("name,rev", LOADABLE)
def test_load_db_prepared(eng, name, rev):
    """The database read back base for base through the results renderer."""
    c = BY_NAME[name]
    m, seqs, ids = expected(name, rev)
    targets = m.seqs
    eng.load_targets([b"ACGT" * 8])
    eng.prep_targets(c.text, c.fasta, rev)
    info = eng.load_db_prepared()
    assert (info.n_targets, info.n_bases, info.n_odd, info.n_text_bytes, info.n_chunks) == (len(targets), sum(len(t) for t in targets), 0, len(seqs), 0)
    assert eng.n_targets == len(targets)
    rests = lc.target_rests(targets)
    hits = [(0, g, p, 0) for g, t in enumerate(targets) for p in range(0, max(len(t), 1), PROBE_LEN)]
    exp = sorted(lc.expected_lines([PROBE_READ], targets, rests, hits))
    eng.set_gene_text(rests)
    eng.load_reads([PROBE_READ])
    nl, nb = eng.results_order(np.array(hits, dtype=np.uint32))
    got = sorted(eng.results_text().splitlines(True))
    assert nl == len(got) == len(hits)
    if got != exp:
        bad = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
        raise AssertionError("line %d of %d: got %r, expected %r" % (bad, len(exp), got[bad:bad + 1], exp[bad:bad + 1]))
    assert (eng.prepared_text(0), eng.prepared_text(1)) == (seqs, ids)  # the prepared texts survive the load


def test_loadable_cases_are_many():
    assert len(LOADABLE) > len(CASES) // 2 and any(BY_NAME[n].fasta for n, _ in LOADABLE) and any(not BY_NAME[n].fasta for n, _ in LOADABLE)


@pytest.mark.parametrize("index", ["picked", "classic"])
@pytest.mark.parametrize("seed", [2, 3])
def test_tuples_of_an_oracle_case(seed, index, monkeypatch):
    """From a raw FASTA in 60-base lines to the resident database with both strands, no text on the host in between:
    the tuples are the oracle's over the oracle's own prepared sequences (seed 3 holds X)."""
    if index == "classic":
        monkeypatch.setenv("MUSC_INDEX", "classic")
    ocfg, reads, targets = make_case(seed)
    cfg = Config(Windows=ocfg.Windows, WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                 MaxReadLength=ocfg.MaxReadLength, MaxMatches=ocfg.MaxMatches, MMTol=ocfg.MMTol, MatchMode=ocfg.MatchMode)
    fasta = b"".join(b">gene%d\n" % g + b"".join(t[i:i + 60] + b"\n" for i in range(0, len(t), 60)) for g, t in enumerate(targets))
    rng = random.Random(seed)
    both = sorted(set(reads) | {orc.revcomp(r) for r in reads if rng.random() < 0.5})  # reads drawn from both strands
    seqs, ids = orc.prep_targets_fasta(fasta, True)
    assert len(seqs) == 2 * len(targets)
    exp = np.array(sorted(orc.match_direct(both, seqs, ocfg)), dtype=np.uint32).reshape(-1, 4)
    assert len(exp) and (exp[:, 1] % 2 == 1).any() and (exp[:, 1] % 2 == 0).any()
    with Engine(0) as e:
        info = e.prep_targets(fasta, True, True)
        assert info.n_targets == len(seqs)
        assert e.prepared_text(1) == b"".join(i + b"\n" for i in ids)
        assert e.load_db_prepared().n_targets == len(seqs)
        e.load_reads(both)
        got = sorted_hits(e.match(cfg, apply_mmtol=False))
        assert index != "classic" or e.stats()["index_kind"] in (0, 3)
        assert got.shape == exp.shape and (got == exp).all()


# ---------------------------------------------------------------- sz_frame

def raw_frame(e, src_ptr, n, src_dev, dst_ptr, cap, dst_dev):
    nout = ctypes.c_uint64(12345)
    rc = e._lib.musc_sz_frame(e._h, src_ptr, n, 1 if src_dev else 0, dst_ptr, cap, 1 if dst_dev else 0, ctypes.byref(nout))
    return rc, int(nout.value), e._lib.musc_last_error(e._h).decode()


@pytest.mark.parametrize("n", [0, 1, 65535, 65536, 65537, 131072, 131073])
def test_sz_frame(eng, torch, n):
    rng = random.Random(n)
    data = bytes(rng.getrandbits(8) for _ in range(n))
    want = sc.frame(data, False)
    assert len(want) == 10 + 8 * ((n + 65535) // 65536) + n and orc.snappy_framed_decode(want) == data
    got = eng.sz_frame(data)  # host to host
    assert got == want
    assert eng.sz_decode(got) == data  # round trip through the device decoder
    src = np.frombuffer(data, dtype=np.uint8)
    sp = src.ctypes.data if n else None
    assert raw_frame(eng, sp, n, False, None, 0, False)[:2] == (0, len(want))  # sizing
    exp = np.frombuffer(want, dtype=np.uint8)
    buf = torch.empty(len(want) + 64, dtype=torch.uint8, device="cuda")
    for k in range(16):
        # the source on the device at offset 15 - k, between guards of its own; the destination at offset k
        d_src, ptr = on_device(torch, data, 15 - k)
        buf.fill_(GUARD)
        torch.cuda.synchronize()
        rc, nout, msg = raw_frame(eng, ptr if k % 4 else sp, n, bool(k % 4), buf.data_ptr() + 16 + k, len(want), True)
        assert (rc, nout) == (0, len(want)), msg
        got = buf.cpu().numpy()
        assert (got[16 + k:16 + k + len(want)] == exp).all(), "offset %d" % k
        assert (got[:16 + k] == GUARD).all() and (got[16 + k + len(want):] == GUARD).all(), "guard bytes, offset %d" % k
    # device to host
    d_src, ptr = on_device(torch, data, 5)
    out = np.full(len(want) + 8, GUARD, dtype=np.uint8)
    rc, nout, msg = raw_frame(eng, ptr, n, True, out.ctypes.data, len(want), False)
    assert (rc, nout) == (0, len(want)) and out[:len(want)].tobytes() == want and (out[len(want):] == GUARD).all()


def test_sz_frame_arguments(eng, torch):
    data = b"ACGT" * 10
    src = np.frombuffer(data, dtype=np.uint8)
    out = np.zeros(64, dtype=np.uint8)
    rc, nout, msg = raw_frame(eng, src.ctypes.data, 40, False, out.ctypes.data, 57, False)
    assert rc == 2 and nout == 58 and "capacity" in msg and not out.any()
    buf = torch.full((128,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert raw_frame(eng, src.ctypes.data, 40, False, buf.data_ptr() + 3, 57, True)[0] == 2
    assert (buf.cpu().numpy() == GUARD).all()
    assert raw_frame(eng, None, 5, False, None, 0, False)[0] == 2
    assert eng._lib.musc_sz_frame(eng._h, None, 0, 0, None, 0, 0, None) == 2
    assert eng.sz_frame(b"") == sc.STREAM_ID
