"""What the walks of tests/walk_cases.py visit, checked on the CPU: none of these conditions depends on the library.  A walk
that never changes PMatch on standing reads, never loads a small read set after the large one, or never asks for a text
it must be refused, would pass on the device and test nothing."""
import itertools

import pytest

import walk_cases as wc

WALKS = {seed: wc.generate(seed) for seed in wc.SEEDS}
EXPECT = {seed: wc.expectations(steps, wc.batch64_of(seed)) for seed, steps in WALKS.items()}
ALL = [(s, e) for seed in wc.SEEDS for s, e in zip(WALKS[seed], EXPECT[seed])]


def test_walks_are_reproducible_and_of_the_committed_length():
    for seed, steps in WALKS.items():
        assert steps == wc.generate(seed) and wc.STEPS <= len(steps) <= wc.STEPS + 40
        assert wc.replay(seed, 17) == steps[:17]
    assert len(wc.SEEDS) >= 12 and any(map(wc.batch64_of, wc.SEEDS)) and not all(map(wc.batch64_of, wc.SEEDS))


def test_every_step_kind_occurs():
    dbs, reads, params = wc.pools()
    seen = {s[0] for s, _ in ALL}
    assert seen == {"db", "reads", "bad_reads", "index", "part", "env", "pass", "replay", "probes", "gtext", "rtext", "order", "rhits",
                    "text", "side", "side_text"}
    assert {s[1:] for s, _ in ALL if s[0] == "db"} == set(itertools.product(dbs, ("ascii", "packed")))
    assert {s[2] for s, _ in ALL if s[0] == "reads"} == set(wc.LOADERS)
    assert {s[1] for s, _ in ALL if s[0] == "reads"} == set(reads)
    assert {s[1] for s, _ in ALL if s[0] == "part"} == {0, 1}
    assert {s[1:] for s, _ in ALL if s[0] == "env"} == {(k, v) for k, vs in wc.ENV_VALUES.items() for v in vs}
    passes = [s for s, e in ALL if s[0] == "pass" and not e["error"]]
    assert {s[1] for s in passes} == set(params) and {s[2] for s in passes} == {False, True}
    assert {s[3] for s in passes} == {"host", "dev", "packed", "compact"} and {s[4] for s in passes} == {1, 2, 3}
    assert {s[1] for s, _ in ALL if s[0] == "replay"} == {False, True}
    assert {s[1] for s, _ in ALL if s[0] == "side_text"} == {0, 1, 2}


def test_a_streamed_load_is_followed_by_its_pass():
    n = 0
    for steps in WALKS.values():
        for a, b in zip(steps, steps[1:] + [("end",)]):
            if a[0] == "reads" and a[2] == "stream":
                assert b[0] == "pass"
                n += 1
    assert n >= 3


def test_every_parameter_set_follows_every_other_on_standing_inputs():
    params = set(wc.pools()[2])
    seen = set()
    for steps, exps in zip(WALKS.values(), EXPECT.values()):
        for (a, ea), (b, eb) in zip(zip(steps, exps), zip(steps[1:], exps[1:])):
            if a[0] == b[0] == "pass" and not ea["error"] and not eb["error"]:
                assert ea["list"][1:3] == eb["list"][1:3]  # nothing between them: same database, same reads
                seen.add((a[1], b[1]))
    missing = {(p, q) for p in params for q in params if p != q} - seen
    assert not missing, sorted(missing)


def test_every_read_set_is_loaded_after_the_large_one():
    after = set()
    for steps in WALKS.values():
        assert steps[1][:2] == ("reads", "big") and steps[2][0] == "pass"
        after |= {s[1] for s in steps[2:] if s[0] == "reads"}
    assert after == set(wc.pools()[1])
    assert {steps[1][2] for steps in WALKS.values()} == set(wc.LOADERS)  # the large set through every loader


def test_a_failed_load_is_followed_by_a_pass_that_is_refused():
    n = 0
    for steps, exps in zip(WALKS.values(), EXPECT.values()):
        for i, s in enumerate(steps):
            if s[0] == "bad_reads":
                assert exps[i]["error"] == wc.E_BAD_LOAD
                assert steps[i + 1][0] == "pass" and exps[i + 1]["error"] == wc.E_NO_READS
                n += 1
    assert n >= 3


def test_a_replay_is_followed_by_order_text_and_another_pass():
    n = 0
    for steps, exps in zip(WALKS.values(), EXPECT.values()):
        for i, s in enumerate(steps):
            if s[0] == "replay" and not exps[i]["error"] and [t[0] for t in steps[i + 1:i + 5]] == ["gtext", "order", "text", "pass"]:
                assert not exps[i + 2]["error"] and not exps[i + 3]["error"]
                assert exps[i + 2]["lines"][0] == exps[i]["list"]  # the order is of the list the replay left
                n += exps[i]["list"][0] == "replay"
    assert n >= 3


@pytest.mark.parametrize("kind", ["replay", "order", "rhits", "text", "side", "side_text"])
def test_each_stage_is_asked_where_it_must_refuse_and_where_it_must_succeed(kind):
    errors = {e["error"] for s, e in ALL if s[0] == kind}
    assert None in errors and len(errors) >= 2, errors
    if kind == "side":
        assert {wc.E_NO_ORDER, wc.E_PASS_AFTER, wc.E_NO_READ_TEXT} <= errors
    if kind == "replay":
        assert {wc.E_NOT_MATCH_LIST, wc.E_PASS_HAD_MMTOL} <= errors
    if kind == "order":
        assert {wc.E_NO_GENE_TEXT, wc.E_NOT_PASS_LIST} <= errors


def test_the_random_walks_reach_every_path_class():
    seen = {c for seed in wc.SEEDS for c in wc.pass_classes(WALKS[seed], wc.batch64_of(seed)) if c}
    assert seen == set(wc.CLASSES)


def test_the_directed_sequence_holds_all_81_ordered_pairs():
    steps = wc.directed()
    exps = wc.expectations(steps)
    pairs, prev, between = set(), None, 0
    for s, e in zip(steps, exps):
        assert not e["error"]
        if s[0] == "pass":
            if prev is not None:
                pairs.add((prev, e["path"]["cls"]))
            prev, between = e["path"]["cls"], 0
        else:
            between += 1
            assert between <= 5 and s[0] in ("db", "reads", "env", "part")
    assert pairs >= set(itertools.product(wc.CLASSES, wc.CLASSES)) and len(set(itertools.product(wc.CLASSES, wc.CLASSES))) == 81
    # each class is what its name says
    paths = {e["path"]["cls"]: e["path"] for e in exps if "path" in e}
    assert (paths["t120"]["kind"], paths["t120"]["family"], paths["t120"]["XM"]) == (1, "k_match_t", 0)
    assert paths["g"]["family"] == "k_match_g" and paths["twide"]["kind"] == 2 and paths["twide"]["WIDE"] == 1
    assert paths["tx_reads"]["XM"] == 1 and paths["tx_db"]["XM"] == 2
    assert (paths["classic"]["kind"], paths["classic"]["family"]) == (0, "k_screen")
    assert (paths["lines"]["kind"], paths["lines"]["family"]) == (3, "k_screen_t")
    assert paths["rstride"]["RW"] == 0 and paths["rstride"]["kind"] == 0 and paths["part"]["nparts"] in (2, 3)


def test_partition_limit_gives_two_to_three_partitions():
    for name, db in wc.pools()[0].items():
        assert len(wc.cut_targets([len(t) for t in db], wc.PART_BASES)) - 1 in (2, 3), name


def test_pools_have_the_shapes_the_walk_is_about():
    dbs, reads, params = wc.pools()
    assert not any(b"X" in t for t in dbs["plain"] + dbs["ragged"])
    xs = [t for t in dbs["xdb"] if b"X" in t]
    assert any(t.count(b"X") == 1 for t in xs) and any(b"XXXXXXX" in t for t in xs)
    assert any(len(t) < 10 for t in dbs["ragged"]) and b"" in dbs["ragged"]
    # the motif's keys sit in more targets than any layout holds inline (3, 2 and 7 entries)
    key = max({t[i:i + 10] for t in dbs["ragged"] for i in range(len(t) - 9)}, key=lambda k: sum(k in t for t in dbs["ragged"]))
    assert sum(key in t for t in dbs["ragged"]) >= 12
    assert len(reads["big"]) == 64 * 6 + 37 and len(reads["r100"]) == len(reads["r100b"]) and reads["r100"] != reads["r100b"]
    assert max(map(len, reads["r150"])) == 150 == min(map(len, reads["r150"])) and max(map(len, reads["r250"])) == 250
    assert all(r.count(b"X") <= 3 for r in reads["rx"]) and any(r.count(b"X") == 3 for r in reads["rx"])
    assert len(reads["one"]) == 1 and reads["none"] == []
    for name, rs in reads.items():
        assert rs == sorted(set(rs)), name
    for name in wc.FIXED_LEN:
        assert {len(r) for r in reads[name]} == {wc.FIXED_LEN[name]} and not any(b"X" in r for r in reads[name])
    # the parameter sets differ from the first in one field each (the small-MaxMatches "first" set in two)
    p0 = params["p0"].__dict__
    for name, p in params.items():
        diff = [k for k in p0 if p.__dict__[k] != p0[k]]
        assert len(diff) == (0 if name == "p0" else 2 if name == "mm6first" else 1), (name, diff)
    assert max(params["win5"].Windows) == max(params["p0"].Windows) != max(params["win30"].Windows)


def test_the_oracle_outputs_tell_the_cached_things_apart():
    dbs, reads, params = wc.pools()
    combos = [(d, r) for d in dbs for r in reads]
    for d, r in combos:
        for p in params:
            assert bool(wc.full_tuples(d, r, p)) == ((r, d) not in wc.EMPTY), (d, r, p)
    full = lambda p, d, r: wc.full_tuples(d, r, p)
    assert any(len({t[0] for t in full("p0", d, r)}) < len(full("p0", d, r)) for d, r in combos)  # reads with several tuples
    assert any(wc.pass_tuples(d, r, "p0", True) != full("p0", d, r) for d, r in combos)
    assert any(wc.pass_tuples(d, r, "tol3", True) != wc.pass_tuples(d, r, "p0", True) for d, r in combos)
    for other in ("pm80", "win5", "win30", "ww12", "dinuc7"):
        assert any(full(other, d, r) != full("p0", d, r) for d, r in combos), other
    assert any(full("win30", d, r) != full("win5", d, r) for d, r in combos)
    assert all(full("p0", d, "r100") != full("p0", d, "r100b") for d in dbs)
    for d, r in combos:
        assert not wc.hot(d, r, "p0") and not wc.hot(d, r, "mm20k")
    assert all(wc.hot(d, "big", "mm6") for d in dbs) and wc.hot("ragged", "r100", "mm6")
    # the replay cuts something, differently for "first" and "best" somewhere
    assert wc.replay_tuples("ragged", "big", "mm6", False) != full("mm6", "ragged", "big")
    assert any(wc.replay_tuples(d, r, "mm6", False) != wc.replay_tuples(d, r, "mm6first", False) for d, r in combos if r != "big")


def test_the_model_agrees_with_itself():
    for seed, steps in WALKS.items():
        assert wc.expectations(steps, wc.batch64_of(seed)) == EXPECT[seed]
    d = wc.directed()
    assert d == wc.directed() and wc.expectations(d) == wc.expectations(d)
