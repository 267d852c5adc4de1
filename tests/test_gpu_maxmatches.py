"""The MaxMatches truncation replayed on the device (musc_maxmatches_apply) against the literal oracle.

Every case of tests/maxmatches_cases.py has at least one (window, key) block above MaxMatches.  The pass runs with
apply_mmtol = 0; apply_maxmatches must then leave exactly the literal oracle's union (apply_mmtol = False) or its
best_filter (True) as the resident list, on every index kind and with the database in two partitions, count the
truncated blocks as the Python model does, and hand that list to the results and side stages."""
import os

import numpy as np
import pytest

from muscato_amd import Config, Engine, MuscatoError
from oracle import literal
from oracle import muscato_oracle as orc

import maxmatches_cases as mc
from test_gpu_results import oracle_text, rests_of
from test_gpu_side import expected as side_expected, tails_of

pytestmark = pytest.mark.gpu

CASES = mc.cases()
KNOBS = ("MUSC_INDEX", "MUSC_DEBUG_MM_HEAP_LDS")
PATHS = [("auto", {}, 0), ("classic", {"MUSC_INDEX": "classic"}, 0), ("lines", {"MUSC_INDEX": "lines"}, 0), ("partitions", {}, 2)]


@pytest.fixture(scope="module")
def eng():
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    with Engine(0) as e:
        yield e
    for k, v in old.items():
        if v is not None:
            os.environ[k] = v


_expect = {}


def expect(case):
    """(literal union, its best_filter, the model's replay), computed once per case."""
    if case.name not in _expect:
        lit = set(literal.match_literal(case.reads, case.targets, case.cfg))
        _expect[case.name] = (lit, orc.best_filter(lit, case.cfg.MMTol), mc.model(case.reads, case.targets, case.cfg))
    return _expect[case.name]


def gcfg(ocfg, part_bases=0):
    return Config(Windows=ocfg.Windows, WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                  MaxReadLength=ocfg.MaxReadLength, MaxMatches=ocfg.MaxMatches, MMTol=ocfg.MMTol, MatchMode=ocfg.MatchMode,
                  DbPartitionBases=part_bases)


def set_env(eng, env):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    eng.reload_env()


def as_set(a):
    t = [tuple(int(v) for v in row) for row in a]
    assert len(set(t)) == len(t), "a tuple twice"
    assert all(x[0] <= y[0] for x, y in zip(t, t[1:])), "the list is not read-major"
    return set(t)


def run(eng, case, apply_mmtol, nparts=0):
    """Load, match with apply_mmtol = 0, replay: (the stage's counts, the new list)."""
    eng.set_partition_bases(0)
    eng.load_targets(case.targets)
    eng.load_reads(case.reads)
    part = (sum(len(t) for t in case.targets) + nparts - 1) // nparts if nparts else 0
    n0 = eng.match_device(gcfg(case.cfg, part), apply_mmtol=False)
    if nparts:
        assert len(eng.partitions()) - 1 >= 2
    assert eng.stats()["n_overflow_blocks"] not in (0, 2 ** 64 - 1)
    got = eng.apply_maxmatches(apply_mmtol)
    eng.set_partition_bases(0)
    hits = eng.hits()
    assert got["nhits"] == len(hits) == eng.stats()["n_hits"] < n0
    return got, as_set(hits)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_parity_on_every_index_kind(eng, case):
    lit, best, rep = expect(case)
    try:
        for name, env, nparts in PATHS:
            set_env(eng, env)
            got, hits = run(eng, case, False, nparts)
            assert hits == lit, name
            assert got["truncated_blocks"] == len(rep.truncated), name
            assert got["suspect_probes"] >= len(rep.truncated), name
            got, hits = run(eng, case, True, nparts)
            assert hits == best, name
            assert got["truncated_blocks"] == len(rep.truncated), name
            assert eng.maxmatches_ms() > 0
    finally:
        set_env(eng, {})


@pytest.mark.parametrize("pick,lds", [("mm6", 4), ("mm65", 16), ("mm1", 1)])
def test_heap_in_global_memory(eng, pick, lds):
    """MUSC_DEBUG_MM_HEAP_LDS below MaxMatches + 1: k_mm_replay keeps the heap in the block's global range."""
    case = next(c for c in CASES if c.cfg.MatchMode == "best" and c.name.endswith(pick))
    assert lds < case.cfg.MaxMatches + 1
    lit, best, rep = expect(case)
    try:
        set_env(eng, {"MUSC_DEBUG_MM_HEAP_LDS": str(lds)})
        got, hits = run(eng, case, False)
        assert hits == lit and got["truncated_blocks"] == len(rep.truncated)
    finally:
        set_env(eng, {})


def test_false_alarms_and_no_suspects(eng):
    """MaxMatches = the largest block: nothing is truncated, whatever the hashed counters suspect -- the list stays as it
    was (apply_mmtol = False) or becomes its best_filter (True), and the counts say so."""
    case = CASES[4]
    rep = expect(case)[2]
    big = max(rep.sizes.values())
    full = orc.match_direct(case.reads, case.targets, case.cfg, check_overflow=False)
    eng.load_targets(case.targets)
    eng.load_reads(case.reads)
    for mm in (big, 10 * big):
        ocfg = orc.Config(**{**case.cfg.__dict__, "MaxMatches": mm})
        for apply_mmtol, exp in ((False, full), (True, orc.best_filter(full, ocfg.MMTol))):
            eng.match_device(gcfg(ocfg), apply_mmtol=False)
            got = eng.apply_maxmatches(apply_mmtol)
            assert got["truncated_blocks"] == 0
            assert as_set(eng.hits()) == exp and got["nhits"] == len(exp)


def test_downstream_stages_read_the_new_list(eng):
    """results_order(None) + results_text and the three side texts after the call are those of the oracle's tuples."""
    base = next(c for c in CASES if c.cfg.MaxMatches == 6 and c.cfg.MatchMode == "best")
    reads = sorted(base.reads)  # the results stage orders by read index: the loaded reads are in bytewise order
    lit = set(literal.match_literal(reads, base.targets, base.cfg))
    kept = sorted(orc.best_filter(lit, base.cfg.MMTol))
    rests = rests_of(base.targets, [b"gene%d" % (g % 7) for g in range(len(base.targets))])
    R = [(r, 1 + i % 3, b"n%d;m%d" % (i, i)) for i, r in enumerate(reads)]
    eng.load_targets(base.targets)
    eng.load_reads(reads)
    eng.set_gene_text(rests)
    eng.set_read_text(tails_of(R))
    eng.match_device(gcfg(base.cfg), apply_mmtol=False)
    got = eng.apply_maxmatches(True)
    assert got["nhits"] == len(kept) and got["truncated_blocks"] >= 1
    exp = oracle_text(reads, base.targets, rests, kept, tails_of(R))
    nl, nb = eng.results_order(None)
    assert (nl, nb) == (len(kept), len(exp))
    assert eng.results_text() == exp
    assert {tuple(int(v) for v in h) for h in eng.results_hits()} == set(kept)
    eng.side_prepare()
    nonmatch, genestats, readstats = side_expected(R, base.targets, rests, kept)
    assert eng.nonmatch_text() == nonmatch
    assert eng.genestats_text() == genestats
    assert eng.readstats_text() == readstats


def test_refused_calls_leave_the_list(eng):
    case = CASES[6]
    cfg = gcfg(case.cfg)
    eng.load_targets(case.targets)
    eng.load_reads(case.reads)
    with pytest.raises(MuscatoError, match=r"\(2\)"):
        eng.apply_maxmatches(True)  # no pass over these reads and targets
    n = eng.match_device(cfg, apply_mmtol=True)
    before = eng.hits()
    with pytest.raises(MuscatoError, match=r"\(2\).*apply_mmtol"):
        eng.apply_maxmatches(True)  # the pass already dropped tuples the replay needs
    assert eng.stats()["n_hits"] == n and np.array_equal(eng.hits(), before)
    eng.match_device(cfg, apply_mmtol=False)
    eng.load_reads(case.reads)
    with pytest.raises(MuscatoError, match=r"\(2\)"):
        eng.apply_maxmatches(True)  # a read load since the pass
    eng.match_device(cfg, apply_mmtol=False)
    eng.load_targets(case.targets)
    with pytest.raises(MuscatoError, match=r"\(2\)"):
        eng.apply_maxmatches(True)  # a database load since the pass
    eng.match_device(cfg, apply_mmtol=False)
    eng.apply_maxmatches(False)
    after = eng.hits()
    with pytest.raises(MuscatoError, match=r"\(2\)"):
        eng.apply_maxmatches(True)  # the list is no longer that of a pass
    assert np.array_equal(eng.hits(), after)


def test_refusal_bound_on_read_length(eng):
    """A loaded read of MUSC_MM_MAX_READ_LEN + 1 bases: code 12, and the list of the pass stays usable; at the bound the
    call is taken."""
    import random
    rng = random.Random(12)
    t = bytes(rng.choice(b"ACGT") for _ in range(1500))
    for L, refused in ((1025, True), (1024, False)):
        reads = sorted({t[7:7 + L], t[100:160]})
        cfg = Config(Windows=[0, 20], WindowWidth=12, PMatch=0.95, MinDinuc=2, MaxReadLength=L, MaxMatches=1000, MMTol=1,
                     MatchMode="best")
        eng.load_targets([t])
        eng.load_reads(reads)
        n = eng.match_device(cfg, apply_mmtol=False)
        before = eng.hits()
        assert n == 2
        if refused:
            with pytest.raises(MuscatoError, match=r"\(12\)"):
                eng.apply_maxmatches(True)
        else:
            assert eng.apply_maxmatches(True) == {"nhits": 2, "suspect_probes": 0, "truncated_blocks": 0}
        assert np.array_equal(eng.hits(), before)
        eng.set_gene_text([b"g\t1500"])
        assert eng.results_order(None)[0] == 2
