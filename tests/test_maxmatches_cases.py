"""The cases of tests/maxmatches_cases.py are what they claim to be, and the Python model of the MaxMatches replay
equals the literal oracle on every one of them (no GPU)."""
import pytest

from oracle import literal
from oracle import muscato_oracle as orc

import maxmatches_cases as mc

CASES = mc.cases()
SHORT = [c for c in CASES if not c.name.startswith("long-")]  # the generator's cases; the long-flank ones beside them


@pytest.fixture(scope="module")
def replays():
    return {c.name: mc.model(c.reads, c.targets, c.cfg) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_truncates_and_model_equals_literal(case, replays):
    rep = replays[case.name]
    assert len(rep.truncated) >= 1
    full = orc.match_direct(case.reads, case.targets, case.cfg, check_overflow=False)
    assert rep.union != full and rep.union < full
    lit = set(literal.match_literal(case.reads, case.targets, case.cfg))
    assert rep.union == lit
    # the per-read selection on top of it
    assert orc.best_filter(rep.union, case.cfg.MMTol) == orc.best_filter(lit, case.cfg.MMTol)


def test_cases_cover_the_edges(replays):
    """Conditions on the inputs: the seeds are chosen so that they hold."""
    long_cases = [c for c in CASES if c not in SHORT]
    assert {c.cfg.MaxMatches for c in SHORT} == {1, 2, 3, 6, 63, 64, 65}
    assert {tuple(c.cfg.Windows) for c in SHORT} == {(0, 5), (0, 3, 6)}
    assert {c.cfg.MatchMode for c in SHORT} == {"best", "first"}
    assert len(long_cases) == 2 and all(len(replays[c.name].truncated) >= 4 for c in long_cases)
    exact = [c.name for c in SHORT if c.cfg.MaxMatches in replays[c.name].sizes.values()]
    plus1 = [c.name for c in SHORT if c.cfg.MaxMatches + 1 in replays[c.name].sizes.values()]
    assert exact, "no case has a block with exactly MaxMatches pairs (it must be left alone)"
    assert plus1, "no case has a block with MaxMatches + 1 pairs (the smallest cut)"
    assert any(replays[c.name].jx0_in_truncated for c in SHORT)
    assert any(replays[c.name].pos_text_order for c in SHORT)
    for c in SHORT:
        assert c.reads != sorted(c.reads), c.name
        assert any(b"X" in r[:4] for r in c.reads) and any(b"X" in r[4:5] for r in c.reads), c.name
        assert any(b"X" in t for t in c.targets), c.name
    # a block over the wave width in both modes (k_mm_replay stages 64 pairs at a time)
    assert any(max(replays[c.name].sizes.values()) > 128 for c in SHORT if c.cfg.MaxMatches >= 63)
