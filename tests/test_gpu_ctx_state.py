"""What a context still holds after each call that can outdate it (generations and stamps): the resident
tuple list across text changes, loads and the MaxMatches replay, the one rule for a load that failed, musc_reload_env,
and create .. destroy cycles in one process.  Every expectation here is the library's documented behaviour from before
the stamps replaced the validity flags; the inputs are test_gpu_results.plain_case (60 reads, 20 targets)."""
import os

import numpy as np
import pytest

from muscato_amd import Config, Engine, MuscatoError, sorted_hits
from oracle import muscato_oracle as orc

from test_gpu_results import plain_case, rests_of

pytestmark = pytest.mark.gpu

NOT_A_PASS_LIST = "resident tuple list is not that of a pass over the reads and the database in hand"
NOT_A_MATCH_LIST = "resident tuple list is not that of a musc_match\\* over the reads and the database in hand"


@pytest.fixture(scope="module")
def case():
    ocfg, reads, targets = plain_case()
    cfg = Config(Windows=ocfg.Windows, WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                 MaxReadLength=ocfg.MaxReadLength, MaxMatches=ocfg.MaxMatches, MMTol=ocfg.MMTol, MatchMode=ocfg.MatchMode)
    rests = rests_of(targets, [b"g%d" % g for g in range(len(targets))])
    tails = [b"%d\tr%d" % (1 + i % 3, i) for i in range(len(reads))]
    full = np.array(sorted(orc.match_direct(reads, targets, ocfg)), dtype=np.uint32).reshape(-1, 4)
    assert len(full) > 40
    return cfg, reads, targets, rests, tails, full


@pytest.fixture()
def eng(case):
    cfg, reads, targets, rests, tails, _ = case
    with Engine(0) as e:
        e.load_targets(targets)
        e.load_reads(reads)
        e.set_gene_text(rests)
        e.set_read_text(tails)
        yield e


def same(got, exp):
    return got.shape == exp.shape and (got == exp).all()


def test_gene_text_after_a_pass_leaves_the_list_usable(eng, case):
    cfg, _, _, rests, _, full = case
    assert eng.match_device(cfg, apply_mmtol=False) == len(full)
    assert eng.results_order(None)[0] == len(full)
    before = eng.results_hits()
    assert same(sorted_hits(before), full)
    eng.set_gene_text(rests)
    with pytest.raises(MuscatoError, match="no ordered list"):
        eng.results_text()  # the order was taken under the old text
    assert eng.results_order(None)[0] == len(full)
    assert same(eng.results_hits(), before)
    assert eng.apply_maxmatches()["nhits"] > 0  # the list is still the pass's


def test_after_the_replay(eng, case):
    cfg, _, _, _, _, full = case
    assert eng.match_device(cfg, apply_mmtol=False) == len(full)
    eng.results_order(None)
    eng.side_prepare()
    n = eng.apply_maxmatches()["nhits"]
    assert 0 < n <= len(full)
    with pytest.raises(MuscatoError, match=NOT_A_MATCH_LIST) as ei:
        eng.apply_maxmatches()
    assert "(2)" in str(ei.value)
    for _ in range(2):  # until a new order, however often it is asked
        with pytest.raises(MuscatoError, match="a pass ran after"):
            eng.side_prepare()
        with pytest.raises(MuscatoError, match="nothing prepared"):
            eng.nonmatch_text()
    assert eng.results_order(None)[0] == n  # the replayed list may be ordered
    eng.side_prepare()
    assert eng.genestats_text() != b""


def test_loads_end_the_standing_of_the_list(eng, case):
    cfg, reads, targets, rests, _, full = case
    for load in (lambda: eng.load_reads(reads[:-1]), lambda: eng.load_reads(reads),
                 lambda: (eng.load_targets(targets), eng.set_gene_text(rests))):
        assert eng.match_device(cfg, apply_mmtol=False) > 0
        assert eng.results_order(None)[0] > 0
        load()
        with pytest.raises(MuscatoError, match=NOT_A_PASS_LIST) as ei:
            eng.results_order(None)
        assert "(2)" in str(ei.value)
        with pytest.raises(MuscatoError, match=NOT_A_MATCH_LIST):
            eng.apply_maxmatches()
        eng.load_reads(reads)
    assert eng.match_device(cfg, apply_mmtol=False) == len(full)
    assert eng.results_order(None)[0] == len(full)


def test_a_failed_load_leaves_no_reads(eng, case):
    cfg, reads, _, _, _, full = case
    assert same(sorted_hits(eng.match(cfg, apply_mmtol=False)), full)
    buf = np.frombuffer(b"".join(reads) + b"\0" * 8, dtype=np.uint8).copy()
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    bad = off.copy()
    bad[0] = 1  # (the first read has 60 bases: the offsets still do not decrease)
    with pytest.raises(MuscatoError, match="read offsets\\[0\\] must be 0") as ei:
        eng.load_reads_arrays(buf, bad)
    assert "(2)" in str(ei.value)
    for _ in range(2):
        with pytest.raises(MuscatoError, match="no reads loaded") as ei:
            eng.match_device(cfg, apply_mmtol=False)
        assert "(4)" in str(ei.value)
    eng.load_reads_arrays(buf, off)
    assert same(sorted_hits(eng.match(cfg, apply_mmtol=False)), full)


def test_reload_env_flips_the_index_and_back(eng, case):
    cfg, _, _, _, _, full = case
    old = os.environ.pop("MUSC_INDEX", None)
    try:
        eng.reload_env()
        kinds = []
        for value in (None, "classic", None):
            if value is None:
                os.environ.pop("MUSC_INDEX", None)
            else:
                os.environ["MUSC_INDEX"] = value
            eng.reload_env()
            for _ in range(2):  # the second pass is the sized one
                assert same(sorted_hits(eng.match(cfg, apply_mmtol=False)), full)
            kinds.append(eng.stats()["index_kind"])
        assert kinds[0] in (1, 2) and kinds[1] in (0, 3) and kinds[2] == kinds[0], kinds
    finally:
        os.environ.pop("MUSC_INDEX", None)
        if old is not None:
            os.environ["MUSC_INDEX"] = old
        eng.reload_env()


def test_twenty_contexts_one_after_the_other(case):
    cfg, reads, targets, rests, tails, full = case
    first = None
    for cycle in range(20):
        with Engine(0) as e:
            e.load_targets(targets)
            e.load_reads(reads)
            e.set_gene_text(rests)
            e.set_read_text(tails)
            n = e.match_device(cfg, apply_mmtol=False)
            e.results_order(None)
            got = [e.results_hits().tobytes(), e.results_text()]
            e.side_prepare()
            got += [e.nonmatch_text(), e.genestats_text(), e.readstats_text()]
            got.append(e.apply_maxmatches()["nhits"])
            got.append(sorted_hits(e.hits()).tobytes())
        if first is None:
            first = got
            assert n == len(full) and got[1].count(b"\n") == n and got[3] != b""
        assert got == first, cycle
