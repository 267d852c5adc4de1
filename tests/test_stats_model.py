"""The counter model (tests/stats_model.py) and the fixtures of tests/test_gpu_stats.py, without a GPU: the model's
accepted count is the oracle's, its quantities are ordered as the pipeline narrows them, and every fixture reaches
every term the counters tell apart -- so that a GPU case that equals the model has not passed on zeros."""
import pytest

from oracle import muscato_oracle as orc

import stats_cases as sc
import stats_model as sm
from cases import make_case


@pytest.mark.parametrize("seed", range(24))
def test_model_on_random_cases(seed):
    """cases.make_case (ragged reads, 1-3 windows, X for every third seed): n_accepted / n_hits are the sizes of
    orc.match_direct's set and of its best + MMTol selection on every index kind; candidates >= fitting candidates >=
    flank survivors >= accepted placements; the flank filter drops no accepted placement; the descriptor bounds are
    ordered; on the fused kinds a read window with an X takes no part."""
    cfg, reads, targets = make_case(seed)
    acc = orc.match_direct(reads, targets, cfg, check_overflow=False)
    acgt = seed % 3 != 0
    for kind in sm.KINDS:
        for apply_mmtol in (False, True):
            e = sm.expected(reads, targets, cfg, kind, acc, apply_mmtol=apply_mmtol)
            m = e["model"]
            assert e["n_accepted"] == len(acc)
            assert e["n_hits"] == (len(orc.best_filter(acc, cfg.MMTol)) if apply_mmtol else len(acc)) == e["staged_tuples"]
            assert e["n_reads"] == len(reads)
            valid = sum(orc.window_valid(r, k, cfg) for r in reads for k in range(len(cfg.Windows)))
            assert e["n_read_windows"] + m["x_windows"] == valid
            if acgt:
                assert m["x_windows"] == 0
            unfit = m["unfit_before_start"] + m["unfit_at_jx0"] + m["unfit_past_end"]
            assert e["n_candidates"] == m["fitting"] + unfit
            if kind in ("ctx", "ctx_wide"):
                assert e["n_pairs"] == m["fitting"] and e["n_descriptors"] == 0
                assert e["n_overflow_entries"] <= e["n_candidates"]
                if acgt:
                    assert m["fitting"] >= m["accepted_triples"]
            elif acgt:
                assert m["fitting"] == e["n_pairs"] + m["flank_rejected"]
                assert m["accepted_not_surviving"] == 0
                assert e["n_pairs"] - m["both_windows"] >= m["accepted_triples"]
                if kind == "lines":
                    assert e["n_descriptors"] == e["n_pairs"]
                else:
                    assert e["n_pairs"] - m["both_windows"] <= e["n_descriptors_lo"] <= e["n_descriptors_hi"] == e["n_pairs"]


def test_fit_rule_is_the_oracles():
    """sm.fits restates the fit rule inside orc.match_direct: with a budget that accepts everything (PMatch 0) and no
    MinDinuc gate, the fitting candidates of one window ARE the oracle's tuples of that window."""
    for seed in range(1, 12):
        cfg, reads, targets = make_case(seed)
        if seed % 3 == 0:
            continue
        for q1 in cfg.Windows:
            c = orc.Config(**dict(cfg.__dict__, Windows=[q1], PMatch=0.0, MinDinuc=0))
            acc = orc.match_direct(reads, targets, c, check_overflow=False)
            e = sm.expected(reads, targets, c, "ctx", acc)
            assert e["model"]["fitting"] == len(acc) == e["n_pairs"], (seed, q1)


FIXTURES = [(p, rs) for p in sc.PATHS for rs in ("ragged", "heavy", "fixed")] + [("t2", "x"), ("t4", "x"), ("wide3", "x")]


@pytest.mark.parametrize("path,rs", FIXTURES)
def test_fixtures_are_not_vacuous(path, rs):
    """Every (path, read set) the GPU module runs, on the model alone.  The one term a fixture lacks: the "fixed" set
    has no length-rejected window, and cannot have one -- the streamed load takes reads of ONE length, and 100 bases
    reach past every window of every path (the last one ends at base 46); its other terms are all there."""
    _, kind, windows = sc.PATHS[path]
    c, reads, full, e = sc.expected_for(path, rs)
    m = e["model"]
    assert len(reads) % 64 != 0
    assert e["n_accepted"] == len(full) > len(reads)
    assert m["dinuc_rejected"] > 0
    if rs != "fixed":
        assert m["len_rejected"] > 0
    else:
        assert m["len_rejected"] == 0 and {len(r) for r in reads} == {100}
    assert m["empty_probes"] > 0
    assert e["n_read_windows"] > 0 and e["n_candidates"] > e["n_read_windows"]
    assert m["unfit_past_end"] > 0 and m["unfit_at_jx0"] > 0
    if len(windows) > 1:
        assert m["unfit_before_start"] > 0
    assert m["fitting"] < e["n_candidates"]
    assert m["multi_tuple_reads"] > 0 and m["max_tuples_per_read"] >= sc.MOTIF_COPIES
    if kind in ("ctx", "ctx_wide"):
        assert e["n_overflow_entries"] > 0 and e["n_pairs"] == m["fitting"] > e["n_accepted"]
        assert e["match_bytes"] > e["match_bytes_strict"] > 0  # (a probe uses less of its line than the line)
        assert (m["x_windows"] > 0) == (rs == "x")
    else:
        assert m["flank_rejected"] > 0 and m["accepted_not_surviving"] == 0
        assert e["n_pairs"] < m["fitting"]
        if len(windows) > 1:
            assert m["both_windows"] > 0
            if kind == "classic64":
                assert e["n_descriptors_lo"] < e["n_descriptors_hi"]
    # the selection removes something: apply_mmtol on and off differ
    assert sc.expected_for(path, rs, apply_mmtol=True)[3]["n_hits"] < e["n_hits"]


def test_bucket_zero_is_not_empty():
    """A probe that takes no part fetches bucket 0 of a direct table (key AAAAAA) and must not be credited with its
    count: that is only visible while bucket 0 holds entries and some read windows take no part -- in the database
    and in its copy with X."""
    c = sc.cfg((0, 20))
    key = b"A" * sc.WW
    for targets in (sc.TARGETS, _xdb()):
        assert len(orc._kmer_index(targets, sc.WW).get(key, ())) > 0
    for rs in ("ragged", "heavy", "fixed", "x"):
        m = sc.expected_for("t2", rs)[3]["model"]
        assert m["len_rejected"] + m["dinuc_rejected"] + m["x_windows"] > 0, rs
    del c


def test_database_with_x_fixture():
    """X in the database (fused path): windows that hold one are not indexed, so the candidates drop below those of the
    X-free database, and the tuples still multi-map."""
    xt = _xdb()
    c, reads, full, e = sc.expected_for("t2", "ragged", targets=xt)
    base = sc.expected_for("t2", "ragged")[3]
    assert 0 < e["n_candidates"] < base["n_candidates"]
    assert e["n_read_windows"] == base["n_read_windows"]
    assert e["n_overflow_entries"] > 0 and e["model"]["max_tuples_per_read"] >= 20
    assert any(h[3] > 0 for h in full.tolist())


_XDB = []


def _xdb():
    if not _XDB:
        _XDB.append(sc.database_with_x())
    return _XDB[0]


def test_heavy_reads_outgrow_a_first_pass():
    """What a first pass provides per batch of n reads before it has seen them -- room for 2 n staged tuples on the
    fused paths, for 4 n descriptors (at least 1024) on the two-kernel path -- is less than the heavy set needs: a fresh
    context that starts with it must grow and repeat a batch."""
    for path in sc.PATHS:
        _, kind, _ = sc.PATHS[path]
        _, reads, _, e = sc.expected_for(path, "heavy")
        n = len(reads)
        if kind in ("ctx", "ctx_wide"):
            assert e["staged_tuples"] > 4 * n
        else:
            assert e.get("n_descriptors_lo", e.get("n_descriptors")) > max(4 * n, 1024)


def test_partitions_sum():
    """Three partitions of whole targets: every partition probes every read window; the candidates -- each in exactly
    one partition's index -- add up to the unpartitioned count, the overflow entries to less (a bucket's inline entries
    exist once per partition); the tables are direct by the rule 4^ww <= 2 x the largest partition's bases."""
    parts = [0, 22, 44, len(sc.TARGETS)]
    assert 4 ** sc.WW <= 2 * max(sum(map(len, sc.TARGETS[a:b])) for a, b in zip(parts, parts[1:]))
    for path in ("t2", "c64_2", "lines_t"):
        one = sc.expected_for(path, "ragged")[3]
        e = sc.expected_for(path, "ragged", parts=parts)[3]
        assert e["n_read_windows"] == 3 * one["n_read_windows"]
        assert e["n_candidates"] == one["n_candidates"] and e["n_pairs"] == one["n_pairs"]
        assert e["n_accepted"] == one["n_accepted"] == e["staged_tuples"]
        if path == "t2":
            assert 0 < e["n_overflow_entries"] < one["n_overflow_entries"]
            assert e["match_bytes"] - one["match_bytes"] == (2 * len(sc.read_set("ragged")) * 25 + 128 * 2 * one["n_read_windows"] -
                                                             40 * (one["n_overflow_entries"] - e["n_overflow_entries"]))
    # with the selection on, every partition's pass keeps its own best + MMTol: more tuples staged than returned
    e = sc.expected_for("t2", "ragged", parts=parts, apply_mmtol=True)[3]
    assert e["staged_tuples"] > e["n_hits"]


def test_index_bytes():
    c = sc.cfg((0, 20))
    whole = sm.index_bytes(sc.TARGETS, c, "ctx")
    assert whole > (4 ** sc.WW + 1) * 128 + sm.ctx_entries_bytes(16, False)
    assert sm.index_bytes(sc.TARGETS, c, "ctx_wide") > whole  # (two inline entries, 60-byte overflow entries)
    assert sm.index_bytes(sc.TARGETS, c, "ctx", 0, 22) < whole
    assert sm.ctx_entries_bytes(3, False) == 128 and sm.ctx_entries_bytes(4, False) == 256 and sm.ctx_entries_bytes(3, True) == 256
