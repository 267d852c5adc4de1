"""The gene file from its raw bytes on the GPU: musc_sz_decode and musc_db_load_text against
tests/sz_cases.py, whose streams, texts and expectations tests/test_sz_cases.py holds to the oracle without a GPU.

sz_decode: every valid stream byte for byte, into device memory at sixteen address offsets between guard bytes; every
invalid one with its code, the number of its chunk and sz.hpp's message, and a destination that is left as it was (so the
ranges of the good neighbours of a bad chunk too).  load_db_text: every line case as plain text on the host, on the
device at sixteen address offsets between bytes that would change the answer if they were read, and framed -- chunks of
65 536 bytes uncompressed and through the test's compressor, short texts in chunks of 7 bytes as well.  The database is
compared with load_targets of the model's targets base for base through the results renderer (tests/loader_cases.py)
and by the tuples of an oracle case on the picked and on the classic index.  Every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest

from muscato_amd import Config, Engine, MuscatoError, sorted_hits
from oracle import muscato_oracle as orc

import loader_cases as lc
import sz_cases as sc
from cases import make_case

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PROBE_LEN = 1000
PROBE_READ = b"ACGT" * (PROBE_LEN // 4)
VALID = [c for c in sc.stream_cases() if c.plain is not None]
INVALID = [c for c in sc.stream_cases() if c.plain is None]


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def raw_sz_decode(e, stream, dst_ptr, capacity, on_device):
    src = np.frombuffer(stream, dtype=np.uint8)
    n = ctypes.c_uint64(12345)
    rc = e._lib.musc_sz_decode(e._h, src.ctypes.data if len(src) else None, len(src), dst_ptr, capacity, 1 if on_device else 0,
                               ctypes.byref(n))
    return rc, int(n.value), e._lib.musc_last_error(e._h).decode()


# ---------------------------------------------------------------- sz_decode

@pytest.mark.parametrize("case", VALID, ids=repr)
def test_sz_decode_valid(eng, torch, case):
    plain, n = case.plain, len(case.plain)
    assert eng.sz_decode(case.stream) == plain
    rc, nout, _ = raw_sz_decode(eng, case.stream, None, 0, 0)  # sizing
    assert (rc, nout) == (0, n)
    buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    exp = np.frombuffer(plain, dtype=np.uint8)
    for k in range(16):
        buf.fill_(GUARD)
        torch.cuda.synchronize()
        rc, nout, msg = raw_sz_decode(eng, case.stream, buf.data_ptr() + 16 + k, n, 1)
        assert (rc, nout) == (0, n), msg
        got = buf.cpu().numpy()
        assert (got[16 + k:16 + k + n] == exp).all(), "offset %d" % k
        assert (got[:16 + k] == GUARD).all() and (got[16 + k + n:] == GUARD).all(), "guard bytes, offset %d" % k


@pytest.mark.parametrize("case", INVALID, ids=repr)
def test_sz_decode_invalid(eng, torch, case):
    """The code, the chunk and the message; and nothing of the stream reaches the destination."""
    cap = 1 << 18
    buf = torch.full((cap + 32,), GUARD, dtype=torch.uint8, device="cuda")
    host = np.full(cap, GUARD, dtype=np.uint8)
    torch.cuda.synchronize()
    want = "musc_sz_decode: chunk %d: %s" % (case.index, case.text)
    for dst, on_device in ((buf.data_ptr() + 16 + 3, 1), (host.ctypes.data, 0)):
        rc, nout, msg = raw_sz_decode(eng, case.stream, dst, cap, on_device)
        assert (rc, msg) == (case.code, want)
    assert (buf.cpu().numpy() == GUARD).all() and (host == GUARD).all()
    with pytest.raises(MuscatoError, match=r"musc_sz_decode failed \(%d\)" % case.code):
        eng.sz_decode(case.stream)
    # a sizing call walks the headers only: it answers for a stream whose blocks are bad
    rc, nout, msg = raw_sz_decode(eng, case.stream, None, 0, 0)
    framing = case.code == 12 or case.text.startswith("sz: ") and case.text != "sz: checksum mismatch" or case.text in (
        "snappy: truncated length", "snappy: bad length")
    assert rc == (case.code if framing else 0), msg


def test_sz_decode_arguments(eng):
    stream = sc.frame(b"ACGT" * 10, True)
    out = np.zeros(64, dtype=np.uint8)
    rc, nout, msg = raw_sz_decode(eng, stream, out.ctypes.data, 39, 0)
    assert rc == 2 and nout == 40 and "capacity" in msg and not out.any()
    assert eng._lib.musc_sz_decode(eng._h, None, 5, None, 0, 0, ctypes.byref(ctypes.c_uint64())) == 2
    assert eng._lib.musc_sz_decode(eng._h, None, 0, None, 0, 0, None) == 2
    assert eng.sz_decode(b"") == b""


# ---------------------------------------------------------------- load_db_text

LINE_CASES = {name: text for name, text, _ in sc.line_cases()}


@functools.lru_cache(maxsize=None)
def model(name):
    targets, n_odd, first = sc.model_targets(LINE_CASES[name])
    rests = lc.target_rests(targets)
    hits = [(0, g, p, 0) for g, t in enumerate(targets) for p in range(0, max(len(t), 1), PROBE_LEN)]
    exp = sorted(lc.expected_lines([PROBE_READ], targets, rests, hits))
    return targets, n_odd, first, rests, hits, exp


@functools.lru_cache(maxsize=None)
def framed(name, form):
    text = LINE_CASES[name]
    if form == "framed-plain":
        return sc.frame(text, False)
    if form == "framed-comp":
        return sc.frame(text, True)
    return sc.frame(text, form == "framed-comp-7", chunk_bytes=7)


def rendered(e, name):
    """Every base of the resident database through the renderer: the sorted lines of one tuple per PROBE_LEN bases."""
    targets, _, _, rests, hits, _ = model(name)
    e.set_gene_text(rests)
    e.load_reads([PROBE_READ])
    nl, nb = e.results_order(np.array(hits, dtype=np.uint32))
    got = e.results_text().splitlines(True)
    assert nl == len(got) == len(hits) and nb == sum(len(x) for x in got)
    return sorted(got)


def check_loaded(e, name, info, n_chunks=None):
    targets, n_odd, first, _, _, exp = model(name)
    text = LINE_CASES[name]
    assert (info.n_targets, info.n_bases, info.n_odd, info.first_odd_target, info.n_text_bytes) == \
        (len(targets), sum(len(t) for t in targets), n_odd, first, len(text))
    if n_chunks is not None:
        assert info.n_chunks == n_chunks
    assert info.ms_decode >= 0 and info.ms_parse > 0
    assert e.n_targets == len(targets)
    got = rendered(e, name)
    if got != exp:
        bad = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
        raise AssertionError("line %d of %d: got %r, expected %r" % (bad, len(exp), got[bad:bad + 1], exp[bad:bad + 1]))


@pytest.mark.parametrize("name", list(LINE_CASES))
def test_load_db_text_plain_host(eng, name):
    """...and the same lines as load_targets of the model's targets renders."""
    eng.load_targets([b"ACGT" * 8])
    info = eng.load_db_text(LINE_CASES[name], framed=0)
    check_loaded(eng, name, info, 0)
    eng.load_targets(model(name)[0])
    assert rendered(eng, name) == model(name)[5]
    info = eng.load_db_text(LINE_CASES[name])  # by the identifier: plain
    check_loaded(eng, name, info, 0)


@pytest.mark.parametrize("name", list(LINE_CASES))
def test_load_db_text_plain_device(eng, torch, name):
    """The text in device memory at sixteen address offsets, between bytes that are bases, tabs and newlines."""
    text = LINE_CASES[name]
    around = np.frombuffer(b"\nAC\tGT\nX\r\n" * ((len(text) + 96) // 10 + 1), dtype=np.uint8)[:len(text) + 64].copy()
    for k in range(16):
        h = around.copy()
        h[16 + k:16 + k + len(text)] = np.frombuffer(text, dtype=np.uint8)
        d = torch.from_numpy(h).cuda()
        torch.cuda.synchronize()
        info = eng.load_db_text((d.data_ptr() + 16 + k, len(text)), framed=0 if k % 2 else -1, on_device=True)
        check_loaded(eng, name, info, 0)


# (chunks of 7 bytes are for the short texts)
FRAMED = [(name, form) for name, text in LINE_CASES.items() for form in ("framed-plain", "framed-comp", "framed-plain-7", "framed-comp-7")
          if len(text) <= 8192 or not form.endswith("-7")]


@pytest.mark.parametrize("name,form", FRAMED)
def test_load_db_text_framed(eng, name, form):
    text = LINE_CASES[name]
    stream = framed(name, form)
    assert orc.snappy_framed_decode(stream) == text
    n_chunks = (len(text) + 6) // 7 if form.endswith("-7") else (len(text) + 65535) // 65536
    check_loaded(eng, name, eng.load_db_text(stream, framed=1), n_chunks)
    check_loaded(eng, name, eng.load_db_text(stream), n_chunks)  # by the identifier: framed


@pytest.mark.parametrize("index", ["picked", "classic"])
@pytest.mark.parametrize("seed", [2, 3])
def test_tuples_of_an_oracle_case(seed, index, monkeypatch):
    """The database from a compressed gene file with id columns answers as the oracle does (seed 3 holds X)."""
    if index == "classic":
        monkeypatch.setenv("MUSC_INDEX", "classic")
    ocfg, reads, targets = make_case(seed)
    cfg = Config(Windows=ocfg.Windows, WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                 MaxReadLength=ocfg.MaxReadLength, MaxMatches=ocfg.MaxMatches, MMTol=ocfg.MMTol, MatchMode=ocfg.MatchMode)
    text = b"".join(t + b"\t%011d\tgene%d\t%d\n" % (g, g, len(t)) for g, t in enumerate(targets))
    exp = np.array(sorted(orc.match_direct(reads, targets, ocfg)), dtype=np.uint32).reshape(-1, 4)
    assert len(exp)
    with Engine(0) as e:
        for stream, fr in ((sc.frame(text, True), -1), (sc.frame(text, False, chunk_bytes=1000), 1), (text, -1)):
            info = e.load_db_text(stream, framed=fr)
            assert info.n_targets == len(targets) and info.n_odd == 0
            e.load_reads(reads)
            got = sorted_hits(e.match(cfg, apply_mmtol=False))
            assert index != "classic" or e.stats()["index_kind"] in (0, 3)  # window-start buckets of either size: two kernels
            assert got.shape == exp.shape and (got == exp).all()


# ---------------------------------------------------------------- codes, and what a context holds afterwards

def test_load_db_text_codes(eng, torch):
    by = {c.name: c for c in sc.stream_cases()}
    for name in ("chunk-65537-plain", "chunk-65537-comp", "mid-bad-offset", "bitflip-crc", "mid-reserved-02", "mid-truncated-chunk"):
        c = by[name]
        with pytest.raises(MuscatoError) as ei:
            eng.load_db_text(c.stream)
        assert str(ei.value) == "musc_db_load_text failed (%d): musc_db_load_text: chunk %d: %s" % (c.code, c.index, c.text)
    for data, fr in ((b"", -1), (b"", 0), (sc.STREAM_ID, -1), (sc.frame(b"", True), 1), (by["only-empty-chunks"].stream, -1)):
        with pytest.raises(MuscatoError, match=r"failed \(2\): database has no sequences"):
            eng.load_db_text(data, framed=fr)
    with pytest.raises(MuscatoError, match=r"failed \(13\)"):
        eng.load_db_text(b"ACGT\nGGA\n", framed=1)  # plain text is no stream
    with pytest.raises(MuscatoError, match=r"failed \(2\)"):
        eng.load_db_text(b"ACGT\n", framed=2)
    d = torch.from_numpy(np.frombuffer(sc.frame(b"ACGT\n", False), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    for fr in (1, -1):
        with pytest.raises(MuscatoError, match=r"failed \(2\): musc_db_load_text: a framed stream must be in host memory"):
            eng.load_db_text((d.data_ptr(), d.numel()), framed=fr, on_device=True)
    assert eng._lib.musc_db_load_text(eng._h, None, 4, 0, 0, None) == 2
    assert eng.load_db_text(b"ACGT\n", framed=0).n_targets == 1  # (and the context is fine afterwards)
    assert eng._lib.musc_db_load_text(eng._h, np.frombuffer(b"GG\n", dtype=np.uint8).ctypes.data, 3, 0, 0, None) == 0  # no info asked for


def test_a_load_over_a_used_context_answers_for_the_new_database():
    """Same reads, the targets in reverse order: the pass after the load must not answer from the index, the gene text or
    the sizes of the database before."""
    ocfg, reads, targets = make_case(2)
    cfg = Config(Windows=ocfg.Windows, WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                 MaxReadLength=ocfg.MaxReadLength, MaxMatches=ocfg.MaxMatches, MMTol=ocfg.MMTol, MatchMode=ocfg.MatchMode)
    other = [t[::-1] if g % 2 else t for g, t in enumerate(targets[::-1])] + [b"ACGTACGTAC"]
    exp_a = np.array(sorted(orc.match_direct(reads, targets, ocfg)), dtype=np.uint32).reshape(-1, 4)
    exp_b = np.array(sorted(orc.match_direct(reads, other, ocfg)), dtype=np.uint32).reshape(-1, 4)
    assert len(exp_a) and len(exp_b) and exp_a.tolist() != exp_b.tolist()
    with Engine(0) as e:
        e.load_targets(targets)
        e.load_reads(reads)
        got = sorted_hits(e.match(cfg, apply_mmtol=False))
        assert got.shape == exp_a.shape and (got == exp_a).all()
        e.load_db_text(sc.frame(b"".join(t + b"\n" for t in other), True))
        got = sorted_hits(e.match(cfg, apply_mmtol=False))
        assert got.shape == exp_b.shape and (got == exp_b).all()
        e.load_db_text(b"\r\n".join(targets), framed=0)
        got = sorted_hits(e.match(cfg, apply_mmtol=False))
        assert got.shape == exp_a.shape and (got == exp_a).all()


def test_a_failed_load_leaves_no_database():
    ocfg, reads, targets = make_case(2)
    cfg = Config(Windows=ocfg.Windows, WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                 MaxReadLength=ocfg.MaxReadLength, MaxMatches=ocfg.MaxMatches, MMTol=ocfg.MMTol, MatchMode=ocfg.MatchMode)
    by = {c.name: c for c in sc.stream_cases()}
    with Engine(0) as e:
        e.load_targets(targets)
        e.load_reads(reads)
        assert len(e.match(cfg))
        with pytest.raises(MuscatoError):
            e.load_targets([])  # any failed database load
        with pytest.raises(MuscatoError) as after_any:
            e.match(cfg)
        for bad in (by["bitflip-data-comp"].stream, by["chunk-65537-comp"].stream, by["mid-too-short"].stream, b""):
            e.load_targets(targets)
            assert len(e.match(cfg))
            with pytest.raises(MuscatoError):
                e.load_db_text(bad)
            with pytest.raises(MuscatoError) as ei:
                e.match(cfg)
            assert str(ei.value) == str(after_any.value) and "no database loaded" in str(ei.value)
            assert e.n_targets == 0
        e.load_db_text(b"\n".join(targets))
        assert len(e.match(cfg))
