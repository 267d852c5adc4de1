"""The bedGraph and the per-target summary made on the device (musc_cov_*) against the brute-force model
of tests/cov_cases.py, which tests/test_cov_cases.py holds to the SAM model's records and to results.txt.

The tuple lists are fed by hand through results_order, as tests/test_gpu_sam.py does; coverage does not depend on the
order of the lines, but the model is given the device's own order (results_hits), so that uniqueness is counted over
the list the device has."""
import ctypes
import random

import numpy as np
import pytest

from muscato_amd import Engine, MuscatoError
from oracle import literal
from oracle import muscato_oracle as orc

import cov_cases as cc
import maxmatches_cases as mc
import sam_cases as sc
from cases import make_case
from test_gpu_results import load, rests_of, staged
from test_gpu_sam import _cfg, eng, feed, knobs  # noqa: F401  (eng is the module's fixture)

pytestmark = pytest.mark.gpu

CASES = cc.seeded_cases()


def model(case, ordered, flags):
    return cc.cov_of(case, ordered, *flags)


def check(eng, case, flags, steps=(), ordered=None):
    """`case` (a sam_cases.Case) under `flags` against the model: the counts, both texts whole and in ranges."""
    ordered = feed(eng, case) if ordered is None else ordered
    bed, summary = model(case, ordered, flags)
    got = eng.cov_prepare(*flags)
    assert got == {"runs": len(bed), "run_bytes": sum(map(len, bed)), "targets": len(summary), "summary_bytes": sum(map(len, summary))}
    assert eng.cov_bedgraph() == b"".join(bed) and eng.cov_summary() == b"".join(summary)
    for text, recs in ((eng.cov_bedgraph, bed), (eng.cov_summary, summary)):
        n = len(recs)
        for step in steps:
            for r0 in range(0, n, step):
                assert text(r0, step) == b"".join(recs[r0:r0 + step]), (step, r0)
        assert text(n, 5) == b"" and text(0, 0) == b""
    return bed, summary


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_cases_against_the_model(eng, case):
    ordered = feed(eng, case.case)
    assert sorted(ordered) == sorted(sc.ordered_hits(case.case))
    for flags in case.flagsets:
        if flags in case.refused:
            continue
        bed, summary = check(eng, case.case, flags, steps=(1, 7, 64), ordered=ordered)
        assert len(summary) > 0


@pytest.fixture(scope="module")
def piles():
    return next(c for c in CASES if c.name == "piles").case


def test_host_and_device_destinations_at_sixteen_alignments(eng, piles):
    import torch
    ordered = feed(eng, piles)
    bed, summary = model(piles, ordered, cc.WEIGHTED)
    got = eng.cov_prepare(weighted=True)
    assert got["runs"] == len(bed) > 64 and eng.cov_bedgraph() == b"".join(bed)
    nb = ctypes.c_uint64()
    for which, recs in ((0, bed), (1, summary)):
        count, whole = len(recs), b"".join(recs)
        for a in range(16):
            r0, cnt = ((0, count), (1, 5), (count - 1, 1))[a % 3]
            want = b"".join(recs[r0:r0 + cnt])
            assert len(want) > 0
            # device memory
            d = torch.full((len(want) + 48,), 0xEE, dtype=torch.uint8, device="cuda")
            assert eng.cov_text_into(which, r0, cnt, d.data_ptr() + 16 + a, len(want), True) == len(want)
            torch.cuda.synchronize()
            h = d.cpu().numpy().tobytes()
            assert h[16 + a:16 + a + len(want)] == want, (which, a)
            assert set(h[:16 + a]) == {0xEE} and set(h[16 + a + len(want):]) == {0xEE}, (which, a)
            # host memory
            buf = np.full(len(want) + 48, 0xEE, dtype=np.uint8)
            assert eng.cov_text_into(which, r0, cnt, buf.ctypes.data + 16 + a, len(want), False) == len(want)
            hb = buf.tobytes()
            assert hb[16 + a:16 + a + len(want)] == want and set(hb[:16 + a]) == {0xEE} and set(hb[16 + a + len(want):]) == {0xEE}
        # one byte short: an error that writes nothing
        buf = np.full(len(whole) + 8, 0xEE, dtype=np.uint8)
        rc = eng._lib.musc_cov_text(eng._h, which, 0, 1 << 62, buf.ctypes.data, len(whole) - 1, 0, ctypes.byref(nb))
        assert rc == 2 and b"capacity" in eng._lib.musc_last_error(eng._h) and nb.value == 0 and set(buf.tolist()) == {0xEE}


@pytest.mark.parametrize("stage_bytes,stage_lines", [(256, 7), (1, 1)])
def test_staged_host_path_in_many_pieces(eng, piles, stage_bytes, stage_lines):
    ordered = feed(eng, piles)
    bed, summary = model(piles, ordered, cc.WEIGHTED)
    eng.cov_prepare(weighted=True)
    with staged(eng, stage_bytes, stage_lines):
        assert eng.cov_bedgraph() == b"".join(bed) and eng.cov_summary() == b"".join(summary)
        assert eng.cov_bedgraph(3, 11) == b"".join(bed[3:14]) and eng.cov_summary(2, 3) == b"".join(summary[2:5])


@pytest.mark.parametrize("kind", ["picked", "classic64"])
def test_list_of_a_real_pass(eng, kind):
    """An oracle case of tests/cases.py: match, order the list the pass left on the device, count."""
    ocfg, reads, targets = make_case(3)
    rests = rests_of(targets, [b"gene_%d" % g for g in range(len(targets))])
    tails = [b"%d\tr%d;x" % (1 + i % 3, i) for i in range(len(reads))]
    absent = (len(targets) - 1,)
    with knobs(eng, **({"MUSC_INDEX": "classic64"} if kind == "classic64" else {})):
        load(eng, reads, targets, rests, tails, absent)
        n = eng.match_device(_cfg(ocfg), apply_mmtol=True)
        assert n > 0 and (kind != "classic64" or eng.stats()["index_kind"] == 0)
        assert eng.results_order(None)[0] > 0
        ordered = [tuple(int(v) for v in h) for h in eng.results_hits()]
        case = sc.Case("pass", reads, targets, rests, ordered, tails, absent)
        for flags in (cc.PLAIN, cc.WEIGHTED, (False, True, True)):
            bed, _ = check(eng, case, flags, ordered=ordered)
            assert len(bed) > 0
        p, t = eng.cov_ms()
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
    bed, _ = check(eng, case, cc.WEIGHTED, ordered=ordered)
    assert len(bed) > 0


@pytest.fixture(scope="module")
def large():
    """Every loop of the stage crossed at least three times by a grid of three blocks: more than 3 x 3 x 256 reads,
    targets, lines, runs and summary records for the grid-stride kernels (twice as many events), more than 3 x 12 records
    for the wave-per-record kernels, and records of more than 3 x 256 bytes for wave_store (a name of 800 bytes)."""
    rng = random.Random(29)
    n = 2400
    targets = [sc.rand_seq(rng, 40, b"ACGT") for _ in range(n)] + [sc.rand_seq(rng, 300, b"ACGT")]
    ln = cc.Lines("large", targets, [b"t%d" % g for g in range(n)] + [b"L" * 800], 29)
    for g in range(n):
        ln.add(g, g % 10, 24, b"%d\tx" % (1 + g % 5))
    ln.add(n, 10, 100, b"3\ta"), ln.add(n, 60, 100, b"4\tb")
    return ln.finish([cc.WEIGHTED]).case


@pytest.mark.parametrize("grid", [3, 1])
def test_stage_grid(eng, large, grid):
    trips = 3 * 3
    assert len(large.reads) >= trips * 256 and len(large.targets) >= trips * 256 and len(large.hits) >= trips * 256
    with knobs(eng, MUSC_DEBUG_STAGE_GRID=str(grid)):
        bed, summary = check(eng, large, cc.WEIGHTED, steps=(1000,))
        check(eng, large, (False, True, True))
    assert len(bed) >= trips * 256 and len(summary) >= trips * 256
    assert max(len(r) for r in bed) >= 3 * 256 and max(len(r) for r in summary) >= 3 * 256
    check(eng, large, cc.WEIGHTED)  # the knob unset: the same bytes


REFUSED = [(c, f) for c in CASES + cc.refusal_cases() for f in c.refused]


@pytest.mark.parametrize("case,flags", REFUSED, ids=lambda v: v.name if isinstance(v, cc.CovCase) else "".join("rwu"[i] if b else "-" for i, b in enumerate(v)))
def test_refusals_leave_the_other_texts_working(eng, case, flags):
    c = case.case
    ordered = feed(eng, c)
    res = eng.results_text()
    try:
        eng.sam_prepare(False)
        sam = eng.sam_header() + eng.sam_text()
    except MuscatoError:
        sam = None  # (a gene text the SAM stage refuses as well)
    with pytest.raises(MuscatoError) as ei:
        eng.cov_prepare(*flags)
    assert "(12)" in str(ei.value)
    for text in (eng.cov_bedgraph, eng.cov_summary):
        with pytest.raises(MuscatoError, match="nothing prepared"):
            text()
    assert eng.results_text() == res and [tuple(int(v) for v in h) for h in eng.results_hits()] == ordered
    if sam is not None:
        assert eng.sam_header() + eng.sam_text() == sam
    if flags[1] or c.name in ("odd_count", "unequal_pair", "even_partner_absent"):
        check(eng, c, cc.PLAIN, ordered=ordered)  # the same inputs are fine without the weights, or without the pairing
    with pytest.raises(MuscatoError) as ei:
        eng._call("musc_cov_prepare", 8, None, None, None, None)
    assert "(2)" in str(ei.value) and "unknown flags" in str(ei.value)


def test_stale_state(eng):
    """No ordered list: code 2.  After the reads, the database, either text or the ordered list is replaced, what was
    prepared is gone, and a correct sequence gives the new inputs' texts; SAM's tables and these do not disturb each
    other."""
    case = next(c for c in CASES if c.name == "unique").case
    other = next(c for c in CASES if c.name == "intervals").case

    def gone(match="nothing prepared"):
        with pytest.raises(MuscatoError, match=match) as ei:
            eng.cov_bedgraph()
        assert "(2)" in str(ei.value)

    def good(c):
        check(eng, c, cc.WEIGHTED)

    with Engine(0) as fresh:
        with pytest.raises(MuscatoError, match="no ordered list") as ei:
            fresh.cov_prepare()
        assert "(2)" in str(ei.value)
        with pytest.raises(MuscatoError, match="nothing prepared"):
            fresh.cov_summary()
    good(case)
    eng.load_reads(case.reads[:-1])
    gone()
    with pytest.raises(MuscatoError, match="no ordered list"):
        eng.cov_prepare()
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
    # both stages over one ordered list, in either order
    ordered = feed(eng, case)
    bed, summary = model(case, ordered, cc.PLAIN)
    eng.sam_prepare(False)
    sam = eng.sam_text()
    eng.cov_prepare()
    assert eng.sam_text() == sam and eng.cov_bedgraph() == b"".join(bed)
    eng.sam_prepare(False)
    assert eng.cov_summary() == b"".join(summary) and eng.sam_text() == sam
