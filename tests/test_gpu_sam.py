"""SAM records and header rendered on the device (musc_sam_*) against the Python model of
tests/sam_cases.py, which tests/test_sam_cases.py holds to results.txt through an independent inverse.

The tuple lists are fed by hand through results_order, as tests/test_gpu_side.py does; the order of the records is the
device's own order of results.txt (results_hits, held to the oracle by tests/test_gpu_results.py), and every byte of
the expected text comes from the model over that order."""
import contextlib
import ctypes
import os
import random

import numpy as np
import pytest

from muscato_amd import Config, Engine, MuscatoError
from oracle import literal
from oracle import muscato_oracle as orc

import maxmatches_cases as mc
import sam_cases as sc
from cases import make_case
from test_gpu_results import load, plain_case, rests_of, staged

pytestmark = pytest.mark.gpu

CASES = sc.seeded_cases()
KNOBS = ("MUSC_DEBUG_STAGE_GRID", "MUSC_INDEX", "MUSC_CONTEXT", "MUSC_DEBUG_STAGE_BYTES", "MUSC_DEBUG_STAGE_LINES")


@pytest.fixture(scope="module")
def eng():
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    with Engine(0) as e:
        yield e
    for k, v in old.items():
        if v is not None:
            os.environ[k] = v


@contextlib.contextmanager
def knobs(eng, **env):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        eng.reload_env()
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
        eng.reload_env()


def feed(eng, case):
    """Load a case and order its tuples -> the ordered tuples, as the device ordered them."""
    load(eng, case.reads, case.targets, case.rests, case.tails, case.absent)
    eng.results_order(np.array(case.hits, dtype=np.uint32).reshape(-1, 4))
    return [tuple(int(v) for v in h) for h in eng.results_hits()]


def model(case, ordered):
    hdr = sc.header(case.targets, case.rests, case.absent, case.rev_pairs)
    return hdr, sc.records(case.reads, case.targets, case.rests, case.tails, ordered, case.rev_pairs, case.absent)


def check(eng, case, steps=()):
    ordered = feed(eng, case)
    assert sorted(ordered) == sorted(sc.ordered_hits(case))
    hdr, recs = model(case, ordered)
    got = eng.sam_prepare(case.rev_pairs)
    assert got == {"records": len(recs), "header_bytes": len(hdr), "record_bytes": sum(len(r) for r in recs)}
    assert eng.sam_header() == hdr
    assert eng.sam_text() == b"".join(recs)
    n = len(recs)
    for step in steps:
        for r0 in range(0, n, step):
            assert eng.sam_text(r0, step) == b"".join(recs[r0:r0 + step]), (step, r0)
    assert eng.sam_text(n, 5) == b"" and eng.sam_text(0, 0) == b""
    return hdr, recs


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_cases_against_the_model(eng, case):
    hdr, recs = check(eng, case, steps=(1, 7, 64))
    assert len(recs) > 0
    # the header in ranges of slots: 0 = @HD, 1 + t = target t, the last = @PG
    nslots = len(case.targets) + 2
    parts = [eng._text_range("musc_sam_text", (0,), s0, 3) for s0 in range(0, nslots, 3)]
    assert b"".join(parts) == hdr and parts[0].startswith(sc.HD)


@pytest.fixture(scope="module")
def mixed():
    """Reads of four lengths on both strands, three lines a read on average, names and counts of several widths."""
    rng = random.Random(21)
    ts = [sc.rand_seq(rng, 90 + 7 * k, b"ACGTX" if k == 2 else b"ACGT") for k in range(4)]
    targets = [x for t in ts for x in (t, orc.revcomp(t))]
    b = sc.Builder("mixed", targets, [n for k in range(4) for n in (b"m%d" % k, b"m%d_r" % k)], rev_pairs=True)
    for i in range(70):
        L = (17, 33, 48, 80)[i % 4]
        for k in range(1 + i % 4):
            g = (3 * i + k) % 8
            pos = (5 * i + 11 * k) % (len(targets[g]) - L + 1 + (6 if i % 9 == 0 else 0))
            S = min(L, len(targets[g]) - pos)
            read = bytearray(targets[g][pos:pos + S] + sc.rand_seq(rng, L - S, b"ACGT"))
            for p in rng.sample(range(L), i % 3):
                read[p] = sc.other(rng, read[p])
            b.add(bytes(read), g, pos, tail=b"%d\tname%d;other" % (10 ** (i % 5), i))
    return b.finish()


def test_host_and_device_destinations_at_sixteen_alignments(eng, mixed):
    import torch
    ordered = feed(eng, mixed)
    hdr, recs = model(mixed, ordered)
    got = eng.sam_prepare(True)
    n = got["records"]
    assert n == len(recs) > 64 and eng.sam_text() == b"".join(recs)
    nb = ctypes.c_uint64()
    for which, whole, count in ((0, hdr, len(mixed.targets) + 2), (1, b"".join(recs), n)):
        for a in range(16):
            r0, cnt = ((0, count), (3, 11), (count - 1, 1))[a % 3]
            if which == 1:
                want = b"".join(recs[r0:r0 + cnt])
            else:
                want = eng._text_range("musc_sam_text", (0,), r0, cnt)
                assert want in hdr
            assert len(want) > 0
            # device memory
            d = torch.full((len(want) + 48,), 0xEE, dtype=torch.uint8, device="cuda")
            assert eng.sam_text_into(which, r0, cnt, d.data_ptr() + 16 + a, len(want), True) == len(want)
            torch.cuda.synchronize()
            h = d.cpu().numpy().tobytes()
            assert h[16 + a:16 + a + len(want)] == want, (which, a)
            assert set(h[:16 + a]) == {0xEE} and set(h[16 + a + len(want):]) == {0xEE}, (which, a)
            # host memory
            buf = np.full(len(want) + 48, 0xEE, dtype=np.uint8)
            assert eng.sam_text_into(which, r0, cnt, buf.ctypes.data + 16 + a, len(want), False) == len(want)
            hb = buf.tobytes()
            assert hb[16 + a:16 + a + len(want)] == want and set(hb[:16 + a]) == {0xEE} and set(hb[16 + a + len(want):]) == {0xEE}
        # one byte short: an error that writes nothing
        buf = np.full(len(whole) + 8, 0xEE, dtype=np.uint8)
        rc = eng._lib.musc_sam_text(eng._h, which, 0, 1 << 62, buf.ctypes.data, len(whole) - 1, 0, ctypes.byref(nb))
        assert rc == 2 and b"capacity" in eng._lib.musc_last_error(eng._h) and nb.value == 0 and set(buf.tolist()) == {0xEE}


@pytest.mark.parametrize("stage_bytes,stage_lines", [(256, 7), (1, 1)])
def test_staged_host_path_in_many_pieces(eng, mixed, stage_bytes, stage_lines):
    ordered = feed(eng, mixed)
    hdr, recs = model(mixed, ordered)
    eng.sam_prepare(True)
    with staged(eng, stage_bytes, stage_lines):
        assert eng.sam_header() == hdr and eng.sam_text() == b"".join(recs)
        assert eng.sam_text(3, 11) == b"".join(recs[3:14])


def _cfg(ocfg):
    return Config(Windows=ocfg.Windows, WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                  MaxReadLength=ocfg.MaxReadLength, MaxMatches=ocfg.MaxMatches, MMTol=ocfg.MMTol, MatchMode=ocfg.MatchMode)


@pytest.mark.parametrize("kind", ["picked", "classic64"])
def test_list_of_a_real_pass(eng, kind):
    """An oracle case of tests/cases.py: match, order the list the pass left on the device, render.  XM is the pass's own
    count, NM the comparison of this stage: they agree wherever the span is the whole read, and both are the oracle's."""
    ocfg, reads, targets = make_case(3)
    rests = rests_of(targets, [b"gene_%d" % g for g in range(len(targets))])
    tails = [b"%d\tr%d;x" % (1 + i % 3, i) for i in range(len(reads))]
    absent = (len(targets) - 1,)
    with knobs(eng, **({"MUSC_INDEX": "classic64"} if kind == "classic64" else {})):
        load(eng, reads, targets, rests, tails, absent)
        n = eng.match_device(_cfg(ocfg), apply_mmtol=True)
        assert n > 0 and (kind != "classic64" or eng.stats()["index_kind"] == 0)
        fed = np.zeros((n, 4), dtype=np.uint32)
        eng.hits_to(fed.ctypes.data, n, False)
        assert eng.results_order(None)[0] > 0
        ordered = [tuple(int(v) for v in h) for h in eng.results_hits()]
        assert sorted(ordered) == sorted(tuple(int(v) for v in h) for h in fed if int(h[1]) not in absent)
        case = sc.Case("pass", reads, targets, rests, ordered, tails, absent)
        hdr, recs = model(case, ordered)
        got = eng.sam_prepare()
        assert got["records"] == len(recs) and eng.sam_header() == hdr and eng.sam_text() == b"".join(recs)
        whole = [r for r in recs if b"S" not in r.split(b"\t")[5]]
        assert whole and all(dict((t[:2], t[5:]) for t in r[:-1].split(b"\t")[11:])[b"NM"] ==
                             dict((t[:2], t[5:]) for t in r[:-1].split(b"\t")[11:])[b"XM"] for r in whole)
        p, t = eng.sam_ms()
        assert p > 0 and t > 0


def test_after_apply_maxmatches(eng):
    base = next(c for c in mc.cases() if c.cfg.MaxMatches == 6 and c.cfg.MatchMode == "best")
    reads = sorted(base.reads)
    kept = orc.best_filter(set(literal.match_literal(reads, base.targets, base.cfg)), base.cfg.MMTol)
    rests = rests_of(base.targets, [b"gene%d" % g for g in range(len(base.targets))])
    tails = [b"%d\tn%d;m" % (1 + i % 3, i) for i in range(len(reads))]
    load(eng, reads, base.targets, rests, tails)
    eng.match_device(_cfg(base.cfg), apply_mmtol=False)
    got = eng.apply_maxmatches(True)
    assert got["nhits"] == len(kept) and got["truncated_blocks"] >= 1
    assert eng.results_order(None)[0] == len(kept)
    ordered = [tuple(int(v) for v in h) for h in eng.results_hits()]
    assert set(ordered) == set(kept)
    case = sc.Case("replayed", reads, base.targets, rests, ordered, tails)
    hdr, recs = model(case, ordered)
    assert eng.sam_prepare()["records"] == len(kept)
    assert eng.sam_header() == hdr and eng.sam_text() == b"".join(recs)


@pytest.fixture(scope="module")
def large():
    """Every loop of the stage crossed at least three times by a grid of three blocks: more than 3 x 3 x 256 reads,
    targets and lines for the grid-stride kernels, more than 3 x 12 records and header slots for the wave-per-record
    kernels, a record of more than 3 x 256 bytes for wave_store, and a span of more than 3 x 2 048 bases for MD."""
    rng = random.Random(22)
    n = 2400
    targets = [sc.rand_seq(rng, 40, b"ACGT") for _ in range(n)] + [sc.rand_seq(rng, 6500, b"ACGT")]
    b = sc.Builder("large", targets, [b"t%d" % g for g in range(n + 1)])
    for g in range(n):
        pos = g % 10
        b.add(b.mutated(rng, g, pos, 24, [g % 24]), g, pos)
    places = sorted(set(rng.sample(range(6300), 60)) | {0, 1, 2047, 2048, 4095, 4096, 6299})
    b.add(b.mutated(rng, n, 100, 6300, places), n, 100)
    b.add(b.mutated(rng, n, 150, 6200, []), n, 150)
    return b.finish()


@pytest.mark.parametrize("grid", [3, 1])
def test_stage_grid(eng, large, grid):
    trips = 3 * 3
    assert len(large.reads) >= trips * 256 and len(large.targets) >= trips * 256 and len(large.hits) >= trips * 256
    assert len(large.hits) >= trips * 4 and len(large.targets) + 2 >= trips * 4
    assert max(len(r) for r in large.reads) >= 3 * 2048 + 1
    with knobs(eng, MUSC_DEBUG_STAGE_GRID=str(grid)):
        hdr, recs = check(eng, large, steps=(1000,))
    assert max(len(r) for r in recs) >= 3 * 256 and len(hdr) >= 3 * 256
    md = max((dict((t[:2], t[5:]) for t in r[:-1].split(b"\t")[11:])[b"MD"] for r in recs), key=len)
    assert md.startswith(b"0") and len(md) > 200
    assert eng.sam_header() == hdr and eng.sam_text() == b"".join(recs)  # the knob unset: the same bytes


@pytest.mark.parametrize("case", sc.refusal_cases(), ids=lambda c: c.name)
def test_refusals_leave_the_other_texts_working(eng, case):
    ordered = feed(eng, case)
    res = eng.results_text()
    try:
        side = eng.side_prepare()
    except MuscatoError:
        side = None  # (a gene text outside the side stage's simple form)
    with pytest.raises(MuscatoError) as ei:
        eng.sam_prepare(case.rev_pairs)
    assert "(12)" in str(ei.value)
    with pytest.raises(MuscatoError, match="nothing prepared"):
        eng.sam_text()
    with pytest.raises(MuscatoError, match="nothing prepared"):
        eng.sam_header()
    assert eng.results_text() == res and [tuple(int(v) for v in h) for h in eng.results_hits()] == ordered
    if side is not None:
        assert len(eng.nonmatch_text()) == side["nonmatch"][1] and len(eng.genestats_text()) == side["genestats"][1]
        assert len(eng.readstats_text()) == side["readstats"][1]
    if case.name in ("odd_count", "unequal_pair", "even_partner_absent"):
        hdr, recs = model(sc.Case(case.name, case.reads, case.targets, case.rests, case.hits, case.tails, case.absent), ordered)
        eng.sam_prepare(False)  # the same inputs are fine without the pairing
        assert eng.sam_header() == hdr and eng.sam_text() == b"".join(recs)


def test_stale_state(eng):
    """No ordered list: code 2.  After the reads, the database, either text or the ordered list is replaced, what was
    prepared is gone, and a correct sequence gives the new inputs' text."""
    case = next(c for c in CASES if c.name == "lines_per_read")
    other = next(c for c in CASES if c.name == "clipped")

    def gone(match="nothing prepared"):
        with pytest.raises(MuscatoError, match=match) as ei:
            eng.sam_text()
        assert "(2)" in str(ei.value)

    def good(c):
        ordered = feed(eng, c)
        hdr, recs = model(c, ordered)
        eng.sam_prepare(c.rev_pairs)
        assert eng.sam_header() == hdr and eng.sam_text() == b"".join(recs)

    with Engine(0) as fresh:
        with pytest.raises(MuscatoError, match="no ordered list") as ei:
            fresh.sam_prepare()
        assert "(2)" in str(ei.value)
        with pytest.raises(MuscatoError, match="nothing prepared"):
            fresh.sam_text()
    good(case)
    eng.load_reads(case.reads[:-1])
    gone()
    with pytest.raises(MuscatoError, match="no ordered list"):
        eng.sam_prepare()
    good(case)
    eng.set_read_text(case.tails)
    gone()
    good(case)
    eng.set_gene_text(case.rests, [g in case.absent for g in range(len(case.targets))])
    gone()
    good(case)
    eng.load_targets(case.targets)
    gone()
    good(case)
    eng.results_order(np.array(case.hits[:5], dtype=np.uint32))
    gone()
    good(other)
    good(case)
