"""Reads of up to 65 535 bases on the two-kernel path against the CPU oracle.

Everything beyond 200 bases of context goes to k_screen -> k_confirm, and a record stride no instance is compiled for
runs the runtime-stride ones: k_screen<0, ..> (Rec<0>: record words read from memory on demand), k_confirm<0, ..> (the
streaming branch of confirm_pair, which walks the words the read has), the budget table beyond its 256 LDS entries.
Cases, reads and the oracle's tuples: tests/long_read_cases.py (coverage conditions and the agreement of the two CPU
oracles: tests/test_long_read_cases.py).  Every case runs on the index the library picks, under MUSC_INDEX=classic and
under MUSC_INDEX=lines, and asserts FIRST which instances ran; every comparison is exact equality of sorted tuple arrays
(hit order is unspecified) or of bytes.

After the match, with nmiss of three and four digits: the 8-byte and 4-byte wire formats (a field that does not fit
fails loudly; 65 535-base reads at PMatch 0.9 reach nmiss 6 553 = 13 bits, which no 32-bit compact word holds beside
gene 3 / pos 17) and results.txt of a real pass, rendered from the resident records and planes."""
import os

import numpy as np
import pytest

import loader_cases as lc
import long_read_cases as lr

pytestmark = pytest.mark.gpu

KNOBS = ("MUSC_INDEX", "MUSC_MATCH", "MUSC_NO_SPEC", "MUSC_DEBUG_CTX_DIRECT", "MUSC_DEBUG_INDEX_BITS", "MUSC_BATCH_READS",
         "MUSC_DEBUG_GRID", "MUSC_CONTEXT", "MUSC_DEBUG_FORCE_WIDE", "MUSC_SCREEN", "MUSC_NO_X_CONTEXT", "MUSC_GRAPH",
         "MUSC_PIPELINE")
INDEXES = ("auto", "classic", "lines")
REFUSED = ("L65535-far",)  # a window may start at base 60 000 at the most


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


class LongEngine:
    """One Engine for the module: the knobs, database and reads it holds."""

    def __init__(self):
        from muscato_amd import Engine
        self.e = Engine(0)
        self.index = None
        self.loaded = None

    def setup(self, index, c):
        if index != self.index:
            for k in KNOBS:
                os.environ.pop(k, None)
            if index != "auto":
                os.environ["MUSC_INDEX"] = index
            self.e.reload_env()
            self.index = index
        if self.loaded != c.name:
            self.e.load_targets(c.targets)
            self.e.set_gene_text(c.rests())
            self.e.load_reads(c.reads)
            self.loaded = c.name
        return self.e

    def run(self, cfg, apply_mmtol):
        from muscato_amd import sorted_hits
        got = sorted_hits(self.e.match(cfg, apply_mmtol=apply_mmtol))
        return got, self.e.stats(), self.e.last_instance()


@pytest.fixture(scope="module")
def le():
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    s = LongEngine()
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


def check_instances(c, index, st, li, what):
    """The runtime-stride instances ran -- with the mask plane on the X variants -- on a classic or a line index."""
    assert st["index_kind"] in (0, 3), (what, st["index_kind"])
    if index != "auto":
        assert st["index_kind"] == {"classic": 0, "lines": 3}[index], (what, st["index_kind"])
    mask, one = int(c.x != ""), int(len(c.windows) <= 2)
    want = {"match": None,
            "screen": {"kernel": "k_screen", "RW": 0, "mask": mask, "one": one, "lines": int(st["index_kind"] == 3)},
            "confirm": {"kernel": "k_confirm", "RW": 0, "mask": mask, "w2": one}}
    for k, w in want.items():
        assert li[k] == w, "%s: launched %s = %s, the case is written for %s" % (what, k, li[k], w)
    assert li["path"] == "two-kernel"


@pytest.mark.parametrize("index", INDEXES)
@pytest.mark.parametrize("name", lr.NAMES)
def test_every_tuple_and_every_pass_form(le, name, index):
    """All accepted tuples, twice (the second pass is sized); best + MMTol 0 and 3; MatchMode first."""
    from muscato_amd import MuscatoError
    c = lr.case(name)
    exp = lr.oracle_hits(name)
    le.setup(index, c)
    what = "%s/%s" % (name, index)
    if name in REFUSED:
        with pytest.raises(MuscatoError, match="bad window start 65500"):
            le.e.match(to_cfg(c), apply_mmtol=False)
        return
    got, st, li = le.run(to_cfg(c), False)
    check_instances(c, index, st, li, what)
    assert_same(got, exp, what + " all tuples")
    print(what, "n_accepted", st["n_accepted"], "n_hits", st["n_hits"], "oracle", len(exp))
    assert st["n_reads"] == len(c.reads) and st["n_accepted"] == st["n_hits"] == len(exp), (what, st)
    assert st["n_overflow_blocks"] == 0
    again, st2, li2 = le.run(to_cfg(c), False)
    check_instances(c, index, st2, li2, what + " repeated")
    assert_same(again, got, what + " repeated pass")
    assert st2["n_accepted"] == st2["n_hits"] == len(exp)
    for mmtol in (0, lr.MMTOL):
        best = lr.best_hits(name, mmtol)
        assert len(best) < len(exp)
        got, st, li = le.run(to_cfg(c, MMTol=mmtol), True)
        check_instances(c, index, st, li, what + " best+%d" % mmtol)
        assert_same(got, best, what + " best + MMTol %d" % mmtol)
        assert st["n_accepted"] == len(exp) and st["n_hits"] == len(best), (what, mmtol, st)
    for mode in ("first", "best"):
        got, st, li = le.run(to_cfg(c, MatchMode=mode), False)
        check_instances(c, index, st, li, what + " " + mode)
        assert_same(got, exp, what + " MatchMode " + mode)


@pytest.mark.parametrize("index", INDEXES)
def test_partitions_split_t0_from_the_last_target(le, index):
    """The database in partitions of at most one T0: T0 and the target the database ends with are matched against
    different indexes, and the tuples are those of one pass."""
    name = "L4099"
    c = lr.case(name)
    e = le.setup(index, c)
    try:
        e.set_partition_bases(len(c.targets[0]))
        for apply_mmtol, exp in ((False, lr.oracle_hits(name)), (True, lr.best_hits(name, lr.MMTOL))):
            got, st, li = le.run(to_cfg(c), apply_mmtol)
            plan = e.partitions()
            assert plan[0] == 0 and plan[-1] == len(c.targets) and len(plan) > 2, plan
            assert plan[1] <= len(c.targets) - 1, plan  # the first partition ends before the last target
            check_instances(c, index, st, li, "partitions/" + index)
            assert_same(got, exp, "partitions/%s apply_mmtol=%s" % (index, apply_mmtol))
            assert st["n_hits"] == len(exp)
    finally:
        e.set_partition_bases(0)
        le.loaded = None


def _packed(e, n, on_device, bits):
    import torch
    if on_device:
        w = torch.zeros(n, dtype=torch.int64, device="cuda")
        e.hits_to_packed(w.data_ptr(), n, True, bits, 0)
        back = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        e.unpack_hits(w.data_ptr(), n, True, bits, back.data_ptr())
        torch.cuda.synchronize()
        return w.cpu().numpy().view(np.uint64), back.cpu().numpy().view(np.uint32)
    w = np.zeros(n, dtype=np.uint64)
    e.hits_to_packed(w.ctypes.data, n, False, bits, 0)
    back = np.zeros((n, 4), dtype=np.uint32)
    e.unpack_hits(w.ctypes.data, n, False, bits, back.ctypes.data)
    return w, back


def _compact(e, n, nr, on_device, bits):
    import torch
    if on_device:
        w = torch.zeros(n, dtype=torch.int32, device="cuda")
        k = torch.zeros(nr, dtype=torch.uint8, device="cuda")
        e.hits_to_compact(w.data_ptr(), n, k.data_ptr(), nr, True, bits)
        torch.cuda.synchronize()
        return w.cpu().numpy().view(np.uint32), k.cpu().numpy()
    w = np.full(n, 0xFFFFFFFF, np.uint32)
    k = np.full(nr, 0xFF, np.uint8)
    e.hits_to_compact(w.ctypes.data, n, k.ctypes.data, nr, False, bits)
    return w, k


@pytest.mark.parametrize("name", ["L4099", "L65535"])
def test_wire_formats_with_nmiss_beyond_a_byte(le, name):
    from muscato_amd import MuscatoError, sorted_hits
    c = lr.case(name)
    exp = lr.oracle_hits(name)
    e = le.setup("auto", c)
    got, st, li = le.run(to_cfg(c), False)
    assert_same(got, exp, name)
    n, nr = len(exp), len(c.reads)
    top = int(exp[:, 3].max())
    assert top == c.budget > 255 and nr < 256 and int(exp[:, 2].max()) < 1 << 17 and len(c.targets) <= 8
    assert (top < 1 << 12) if name == "L4099" else (top >> 12 == 1)  # 12 bits hold every nmiss of the first; the second needs 13
    words = {}
    for on_device in (False, True):
        buf = np.zeros(n, dtype=np.uint64)
        with pytest.raises(MuscatoError, match="does not fit"):
            e.hits_to_packed(buf.ctypes.data, n, False, [8, 3, 17, 8], 0)
        w, back = _packed(e, n, on_device, [8, 3, 17, 13])
        assert_same(sorted_hits(back), exp, "%s packed, device=%s" % (name, on_device))
        assert ((w & np.uint64(0x1FFF)) == back[:, 3]).all()
        words[on_device] = w
    assert (words[False] == words[True]).all()
    for on_device in (False, True):
        if name == "L4099":
            w, k = _compact(e, n, nr, on_device, [3, 17, 12])
            assert (k == np.bincount(exp[:, 0], minlength=nr)).all()
            dec = np.stack([np.repeat(np.arange(nr, dtype=np.uint32), k), w >> 29, (w >> 12) & 0x1FFFF, w & 0xFFF], axis=1).astype(np.uint32)
            assert_same(sorted_hits(dec), exp, "%s compact, device=%s" % (name, on_device))
            with pytest.raises(MuscatoError, match="does not fit"):
                _compact(e, n, nr, on_device, [3, 17, 8])
        else:
            # nmiss up to 6 553 needs 13 bits: 3 + 17 + 13 is more than the word has, and 12 bits lose tuples
            with pytest.raises(MuscatoError, match="add up to 33 > 32 bits"):
                _compact(e, n, nr, on_device, [3, 17, 13])
            with pytest.raises(MuscatoError, match="does not fit"):
                _compact(e, n, nr, on_device, [3, 17, 12])


@pytest.mark.parametrize("name", ["L4099-xt", "L65535", "L65535-xr"])
def test_results_text_of_a_real_pass(le, name):
    """results_order + results_text on the tuples a pass left on the device: a 65 535-base read and its span beside a
    four-digit nmiss, X on either side rendered from the mask planes."""
    from muscato_amd import sorted_hits
    c = lr.case(name)
    e = le.setup("auto", c)
    for apply_mmtol, exp in ((False, lr.oracle_hits(name)), (True, lr.best_hits(name, lr.MMTOL))):
        got, st, li = le.run(to_cfg(c), apply_mmtol)
        assert_same(got, exp, name)
        nl, nb = e.results_order()
        ordered = e.results_hits()
        assert nl == len(exp)
        assert_same(sorted_hits(ordered), exp, name + " ordered")
        lines = lc.expected_lines(c.reads, c.targets, c.rests(), ordered.tolist())
        text = e.results_text()
        assert nb == len(text) == sum(map(len, lines))
        got_lines = text.splitlines(True)
        bad = next((i for i, (a, b) in enumerate(zip(got_lines, lines)) if a != b), None)
        assert bad is None and len(got_lines) == len(lines), "line %s of %d differs (tuple %s)" % (bad, len(lines), ordered[bad or 0].tolist())
        if apply_mmtol is False and c.lmax == 65535:
            assert any(len(c.reads[r]) == 65535 and nx > 999 for r, g, p, nx in ordered.tolist())
