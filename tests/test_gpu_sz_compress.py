"""The compressing writer of framed snappy streams on the GPU: musc_sz_compress and musc_targets_prep_sz
against tests/sz_compress_cases.py, whose model and cases tests/test_sz_compress_cases.py holds without a GPU.

Every case: Engine.sz_compress byte-equal to the model, with the source and the destination on the host and on the
device, each at sixteen alignments between guard bytes that must survive; Engine.sz_decode -- the decoder kernel that
was there before -- of the result gives the plain bytes back.  The nine- and ten-chunk cases again on grids of three
blocks and of one (MUSC_DEBUG_STAGE_GRID).  The sizing call, the refusals and what they leave.  prepared_sz in both
modes, and the tuples of an oracle case over a gene stream that was compressed on the device."""
import contextlib
import ctypes
import os
import random

import numpy as np
import pytest

from muscato_amd import Config, Engine, MuscatoError, sorted_hits
from oracle import muscato_oracle as orc

import sz_cases as sc
import sz_compress_cases as zc
from cases import make_case

pytestmark = pytest.mark.gpu

GUARD = 0xA5
AROUND = b"\n>\t"  # around a text on the device: bytes that would change the answer if they were read
KNOB = "MUSC_DEBUG_STAGE_GRID"
CASES = zc.cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def eng():
    old = os.environ.pop(KNOB, None)
    try:
        with Engine(0) as e:
            yield e
    finally:
        os.environ.pop(KNOB, None)
        if old is not None:
            os.environ[KNOB] = old


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@contextlib.contextmanager
def stage_grid(eng, knob):
    os.environ[KNOB] = str(knob)
    try:
        eng.reload_env()
        yield
    finally:
        os.environ.pop(KNOB, None)
        eng.reload_env()


def on_device(torch, text, k):
    """`text` in device memory at address offset k (mod 16), AROUND on both sides: the tensor and the pointer."""
    h = np.frombuffer(AROUND * ((len(text) + 96) // len(AROUND) + 1), dtype=np.uint8)[:len(text) + 64].copy()
    h[16 + k:16 + k + len(text)] = np.frombuffer(text, dtype=np.uint8)
    d = torch.from_numpy(h).cuda()
    torch.cuda.synchronize()
    assert d.data_ptr() % 16 == 0
    return d, d.data_ptr() + 16 + k


def raw_compress(e, src_ptr, n, src_dev, dst_ptr, cap, dst_dev):
    nout = ctypes.c_uint64(12345)
    rc = e._lib.musc_sz_compress(e._h, src_ptr, n, 1 if src_dev else 0, dst_ptr, cap, 1 if dst_dev else 0, ctypes.byref(nout))
    return rc, int(nout.value), e._lib.musc_last_error(e._h).decode()


def same(got, want, what):
    if got != want:
        bad = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError("%s: byte %d of %d / %d: got %r, expected %r" % (what, bad, len(got), len(want), got[bad:bad + 16], want[bad:bad + 16]))


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_sz_compress(eng, torch, name):
    data = BY_NAME[name].plain
    n = len(data)
    want = zc.model(data)
    bound = zc.bound(n)
    assert len(want) <= bound
    same(eng.sz_compress(data), want, "host to host")
    assert eng.sz_decode(want) == data  # the decoder kernel on the new encoder's output
    src = np.frombuffer(data, dtype=np.uint8)
    sp = src.ctypes.data if n else None
    assert raw_compress(eng, sp, n, False, None, 0, False)[:2] == (0, bound)  # sizing: the bound
    exp = np.frombuffer(want, dtype=np.uint8)
    buf = torch.empty(bound + 64, dtype=torch.uint8, device="cuda")
    for k in range(16):
        # the source at offset 15 - k (on the device between guards of its own, or on the host); the destination on the device at offset k
        d_src, ptr = on_device(torch, data, 15 - k)
        buf.fill_(GUARD)
        torch.cuda.synchronize()
        rc, nout, msg = raw_compress(eng, ptr if k % 4 else sp, n, bool(k % 4), buf.data_ptr() + 16 + k, bound, True)
        assert (rc, nout) == (0, len(want)), msg
        got = buf.cpu().numpy()
        same(got[16 + k:16 + k + len(want)].tobytes(), want, "destination offset %d" % k)
        assert (got[:16 + k] == GUARD).all() and (got[16 + k + len(want):] == GUARD).all(), "guard bytes, offset %d" % k
        # device to host, the destination at offset k of a host buffer
        out = np.full(bound + 32, GUARD, dtype=np.uint8)
        rc, nout, msg = raw_compress(eng, ptr, n, True, out.ctypes.data + k, bound, False)
        assert (rc, nout) == (0, len(want)), msg
        same(out[k:k + len(want)].tobytes(), want, "device to host, offset %d" % k)
        assert (out[:k] == GUARD).all() and (out[k + len(want):] == GUARD).all(), "host guard bytes, offset %d" % k


@pytest.mark.parametrize("knob", [3, 1])
@pytest.mark.parametrize("name", ["nine-chunks", "ten-chunks-ids", "mixed-chunks"])
def test_sz_compress_on_a_small_grid(eng, torch, name, knob):
    """A grid of three blocks and of one: every workgroup of k_sz_compress and k_sz_gather crosses its chunk loop."""
    data = BY_NAME[name].plain
    want = zc.model(data)
    nch = (len(data) + zc.CHUNK - 1) // zc.CHUNK
    if name != "mixed-chunks":
        assert nch >= 3 * 3, "%d chunks give a grid of three blocks fewer than three trips" % nch
    d_src, ptr = on_device(torch, data, 7)
    buf = torch.full((zc.bound(len(data)) + 64,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with stage_grid(eng, knob):
        same(eng.sz_compress(data), want, "host to host")
        rc, nout, msg = raw_compress(eng, ptr, len(data), True, buf.data_ptr() + 16 + 3, zc.bound(len(data)), True)
    assert (rc, nout) == (0, len(want)), msg
    got = buf.cpu().numpy()
    same(got[19:19 + len(want)].tobytes(), want, "device to device")
    assert (got[:19] == GUARD).all() and (got[19 + len(want):] == GUARD).all()


def test_sz_compress_arguments(eng, torch):
    data = b"ACGT" * 10
    src = np.frombuffer(data, dtype=np.uint8)
    out = np.zeros(64, dtype=np.uint8)
    assert zc.bound(40) == 58
    rc, nout, msg = raw_compress(eng, src.ctypes.data, 40, False, out.ctypes.data, 57, False)  # one below the bound
    assert rc == 2 and "capacity" in msg and not out.any()
    buf = torch.full((128,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert raw_compress(eng, src.ctypes.data, 40, False, buf.data_ptr() + 3, 57, True)[0] == 2
    assert (buf.cpu().numpy() == GUARD).all()
    assert raw_compress(eng, None, 5, False, None, 0, False)[0] == 2  # NULL input with bytes
    assert raw_compress(eng, None, 5, False, out.ctypes.data, 64, False)[0] == 2 and not out.any()
    assert eng._lib.musc_sz_compress(eng._h, None, 0, 0, None, 0, 0, None) == 2
    assert eng.sz_compress(b"") == sc.STREAM_ID
    rc, nout, msg = raw_compress(eng, src.ctypes.data, 40, False, out.ctypes.data, 58, False)
    assert (rc, nout) == (0, len(zc.model(data))) and out[:nout].tobytes() == zc.model(data) and not out[nout:].any()


def test_prepared_sz(eng):
    """Both modes against sz_frame / sz_compress of prepared_text; without a prepared text: 2."""
    eng.free_prepared()
    with pytest.raises(MuscatoError, match=r"failed \(2\)"):
        eng.prepared_sz(0, True)
    with pytest.raises(MuscatoError, match=r"failed \(2\)"):
        eng.prepared_sz(1, False)
    rng = random.Random(31)
    genes = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(50, 4000))) for _ in range(90)]
    genes[7] = genes[3][:900] + genes[7]  # (something to find)
    fasta = b"".join(b">gene%d some text\n" % g + b"".join(t[i:i + 70] + b"\n" for i in range(0, len(t), 70)) for g, t in enumerate(genes))
    for rev in (False, True):
        eng.prep_targets(fasta, True, rev)
        for which in (0, 1):
            text = eng.prepared_text(which)
            assert len(text) > (100000 if which == 0 else 1000)
            assert eng.prepared_sz(which, False) == eng.sz_frame(text) == sc.frame(text, False)
            got = eng.prepared_sz(which, True)
            same(got, zc.model(text), "prepared text %d" % which)
            assert got == eng.sz_compress(text) and len(got) < len(text) and sc.ref_decode(got) == text
        with pytest.raises(MuscatoError, match=r"failed \(2\)"):
            eng.prepared_sz(2, True)
    eng.prep_targets(b"", True, False)  # two empty texts
    assert eng.prepared_sz(0, True) == eng.prepared_sz(1, False) == sc.STREAM_ID
    eng.free_prepared()
    with pytest.raises(MuscatoError, match=r"failed \(2\)"):
        eng.prepared_sz(0, False)


@pytest.mark.parametrize("seed", [2, 3])
def test_tuples_over_a_compressed_gene_stream(seed):
    """load_db_text of a gene stream that the device compressed: the oracle's tuples, the same as from the stored stream."""
    ocfg, reads, targets = make_case(seed)
    cfg = Config(Windows=ocfg.Windows, WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                 MaxReadLength=ocfg.MaxReadLength, MaxMatches=ocfg.MaxMatches, MMTol=ocfg.MMTol, MatchMode=ocfg.MatchMode)
    text = b"".join(t + b"\n" for t in targets)
    exp = np.array(sorted(orc.match_direct(sorted(set(reads)), targets, ocfg)), dtype=np.uint32).reshape(-1, 4)
    assert len(exp)
    with Engine(0) as e:
        streams = (e.sz_compress(text), e.sz_frame(text))
        assert streams[0] == zc.model(text) and len(streams[0]) < len(streams[1])
        got = []
        for s in streams:
            assert e.load_db_text(s).n_targets == len(targets)
            e.load_reads(sorted(set(reads)))
            got.append(sorted_hits(e.match(cfg, apply_mmtol=False)))
        assert got[0].shape == exp.shape and (got[0] == exp).all() and (got[1] == got[0]).all()
