"""musc_stats against an independent model.  Every roofline figure of the project is a musc_stats byte count divided by a
time; the other GPU modules compare those counters with themselves (one instance against another, a repeat against the
first pass, replay against launches).  Here every counter the header defines is held to tests/stats_model.py -- the
oracle's own window gate, k-mer index and fit rule, recounted on the CPU -- on every path (k_match_t with one, two and
four windows and on wide buckets, k_match_g, 64-byte buckets with one and two windows, line buckets through k_screen_t
and k_screen) and in every way a pass can run: the first, careful pass of a fresh context, the sized pass after it,
hipGraph capture and replay, one batch and several with a ragged last one, a streamed load, a first pass that must
grow its buffers and repeat a batch, the exact repeat of a pass whose MaxMatches screening was inconclusive (and the
capture and replay that follow it with MUSC_GRAPH=1), the selection on and off, partitions, X on either side, and a hashed table (bounds).

The database (tests/stats_cases.py) is 25 kbase with WindowWidth 6: every table is direct by the documented rules, so
the comparisons are equalities.  last_instance() is asserted before any counter: a case that ran on another path than
the one it names fails instead of passing."""
import os

import numpy as np
import pytest

import stats_cases as sc
import stats_model as sm

pytestmark = pytest.mark.gpu

KNOBS = ("MUSC_INDEX", "MUSC_MATCH", "MUSC_SCREEN", "MUSC_CONTEXT", "MUSC_NO_SPEC", "MUSC_DEBUG_CTX_DIRECT", "MUSC_DEBUG_INDEX_BITS",
         "MUSC_BATCH_READS", "MUSC_DEBUG_GRID", "MUSC_DEBUG_FORCE_WIDE", "MUSC_GRAPH", "MUSC_PIPELINE", "MUSC_DEBUG_SYNC",
         "MUSC_NO_X_CONTEXT", "MUSC_DEBUG_INDEX_BUDGET_MB")
BATCH = 1024
FUSED = ("t1", "t2", "t4", "wide3", "dma")
# the instance each path must run on: (last_instance key, kernel, template arguments)
INSTANCE = {
    "t1": ("match", "k_match_t", dict(RW=8, W=1, XM=0, WIDE=0, SG=0)),
    "t2": ("match", "k_match_t", dict(RW=8, W=2, XM=0, WIDE=0, SG=0)),
    "t4": ("match", "k_match_t", dict(RW=8, W=4, XM=0, WIDE=0, SG=0)),
    "wide3": ("match", "k_match_t", dict(RW=8, W=3, XM=0, WIDE=1, SG=0)),
    "dma": ("match", "k_match_g", dict(RW=8, SG=0)),
    "c64_1": ("screen", "k_screen", dict(RW=8, mask=0, one=1, lines=0)),
    "c64_2": ("screen", "k_screen", dict(RW=8, mask=0, one=1, lines=0)),
    "lines_t": ("screen", "k_screen_t", dict(RW=8)),
    "lines_wg": ("screen", "k_screen", dict(RW=8, mask=0, one=1, lines=1)),
}
# the fields that must EQUAL the model on a direct table without X, per path family: none may be left out of a case
EXACT_FUSED = ("n_reads", "n_read_windows", "n_candidates", "n_pairs", "n_descriptors", "n_accepted", "n_hits", "n_overflow_entries",
               "match_bytes", "match_bytes_strict", "confirm_bytes", "confirm_launches", "index_kind")
EXACT_TWO = ("n_reads", "n_read_windows", "n_candidates", "n_pairs", "n_accepted", "n_hits", "n_overflow_entries", "match_bytes",
             "match_bytes_strict", "match_launches", "index_kind")


def to_cfg(c):
    from muscato_amd import Config
    return Config(Windows=list(c.Windows), WindowWidth=c.WindowWidth, PMatch=c.PMatch, MinDinuc=c.MinDinuc,
                  MaxReadLength=c.MaxReadLength, MaxMatches=c.MaxMatches, MMTol=c.MMTol, MatchMode=c.MatchMode)


_ENGINES = []


@pytest.fixture(autouse=True)
def _close_engines():
    yield
    while _ENGINES:
        _ENGINES.pop().close()


def engine(path, batch=None, graph=False, extra=None, targets=None):
    """A fresh Engine on `path` (the knobs are read by musc_init; the environment is put back at once), the database
    loaded.  Closed when the test ends."""
    from muscato_amd import Engine
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(sc.PATHS[path][0])
    if batch:
        os.environ["MUSC_BATCH_READS"] = str(batch)
    if graph:
        os.environ["MUSC_GRAPH"] = "1"
    os.environ.update(extra or {})
    try:
        e = Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    _ENGINES.append(e)
    e.load_targets(sc.TARGETS if targets is None else targets)
    return e


def run(e, c, apply_mmtol):
    from muscato_amd import sorted_hits
    got = sorted_hits(e.match(to_cfg(c), apply_mmtol=apply_mmtol))
    return got, e.stats(), e.last_instance()


def check_instance(path, inst, what, **over):
    key, kernel, args = INSTANCE[path]
    args = dict(args, **over)
    assert inst["path"] == ("fused" if key == "match" else "two-kernel"), (what, inst)
    d = inst[key]
    assert d is not None and d["kernel"] == kernel and {k: d[k] for k in args} == args, (what, d)


def check(path, st, inst, exp, n_batches, what, hashed=False, graph_pass=False, **over):
    """The counters of one pass against the model's: the instance first, then every exact field of the path's family, the
    launch counts, and the descriptor bracket on 64-byte buckets.  hashed: colliding keys are walked -- candidates and
    overflow entries exceed the model, and so do the pairs (fused: every fitting entry is compared; two-kernel: the screen
    never compares the key, so a colliding entry that fits and passes the flank filter becomes a pair) -- and the bytes
    follow the header's formulas on the REPORTED counts; everything else stays exact.  graph_pass: the pass was captured
    or replayed as a hipGraph, whose launches carry no per-kernel events (ms_screen is 0)."""
    check_instance(path, inst, what, **over)
    print(what, {k: st[k] for k in st if not k.startswith("ms_")})
    fused = path in FUSED
    ge = ("n_candidates", "n_pairs") + (("n_overflow_entries",) if fused else ()) if hashed else ()
    for k in EXACT_FUSED if fused else EXACT_TWO:
        if k in ge:
            assert st[k] > exp[k], (what, k, st[k], exp[k])  # (1024 buckets for 4096 keys)
        elif hashed and fused and k in ("match_bytes", "match_bytes_strict"):
            continue  # (by the formulas, below)
        else:
            assert st[k] == exp[k], (what, k, st[k], exp[k])
    assert st["n_batches"] == n_batches, (what, st["n_batches"], n_batches)
    if fused:
        assert st["match_launches"] == n_batches, (what, st["match_launches"])
        rec_b, ent_b = exp["record_bytes"], exp["entry_bytes"]
        if hashed:
            assert st["match_bytes"] == (st["n_reads"] * rec_b + 128 * st["n_read_windows"] + ent_b * st["n_overflow_entries"] +
                                         16 * exp["staged_tuples"]), (what, st["match_bytes"])
            assert st["match_bytes_strict"] == (st["n_reads"] * rec_b + 8 * st["n_read_windows"] + ent_b * st["n_candidates"] +
                                                16 * exp["staged_tuples"]), (what, st["match_bytes_strict"])
        assert (st["ms_screen"] == 0) == graph_pass, (what, st["ms_screen"])
    else:
        assert st["confirm_launches"] == n_batches, (what, st["confirm_launches"])
        if "n_descriptors" in exp:
            assert st["n_descriptors"] == st["n_pairs"], (what, st["n_descriptors"], st["n_pairs"])
            assert hashed or st["n_descriptors"] == exp["n_descriptors"], (what, st["n_descriptors"], exp["n_descriptors"])
        else:
            assert exp["n_descriptors_lo"] <= st["n_descriptors"] <= st["n_pairs"], (what, st["n_descriptors"], exp)
            if not hashed:
                assert st["n_descriptors"] <= exp["n_descriptors_hi"], (what, st["n_descriptors"], exp)
                # n_pairs - n_descriptors = the two-window descriptors: at most the placements found through both windows
                assert st["n_pairs"] - st["n_descriptors"] <= exp["model"]["both_windows"], what
        assert st["confirm_bytes"] == st["n_descriptors"] * exp["descriptor_bytes"] + 16 * exp["staged_tuples"], (what, st["confirm_bytes"])


def same(got, exp, what):
    assert got.shape == exp.shape, "%s: tuple count differs: gpu %d vs oracle %d" % (what, len(got), len(exp))
    assert (got == exp).all(), what


def best_of(full, c):
    from oracle import muscato_oracle as orc
    return sm.as_hits(orc.best_filter(map(tuple, full.tolist()), c.MMTol))


# (MUSC_GRAPH=1 concerns the fused pass alone: the two-kernel path has no graph, its cases run launch by launch)
FORMS = [(p, b, g) for p in sc.PATHS for b in (None, BATCH) for g in ((False, True) if p in FUSED else (False,))]


@pytest.mark.parametrize("path,batch,graph", FORMS,
                         ids=["%s-%s-%s" % (p, "batch-1024" if b else "one-batch", "graph" if g else "launches") for p, b, g in FORMS])
def test_pass_forms(path, batch, graph):
    """A fresh context: the careful first pass, the identical pass after it (sized; with MUSC_GRAPH=1 the capture),
    a third (sized again; the replay), then the selection on, twice.  One batch, or batches of 1024 reads with a ragged
    last one.  Every pass reports the model's counters and the oracle's tuples.  That a sized pass with MUSC_GRAPH=1
    did run as a hipGraph, and not launch by launch after a failed capture, shows in ms_screen: a graph's launches
    carry no per-kernel events."""
    e = engine(path, batch=batch, graph=graph)
    c, reads, full, exp = sc.expected_for(path, "ragged")
    _, _, _, exp_best = sc.expected_for(path, "ragged", apply_mmtol=True)
    best = best_of(full, c)
    nb = sm.uniform_batches(len(reads), batch) if batch else 1
    assert not batch or (nb == 3 and len(reads) % batch)
    e.load_reads(reads)
    for i, form in enumerate(("careful", "sized", "sized again")):
        got, st, inst = run(e, c, False)
        what = "%s %s %s %s" % (path, batch, "graph" if graph else "launches", form)
        check(path, st, inst, exp, nb, what, graph_pass=graph and i > 0)
        same(got, full, what)
    for form in ("careful", "sized"):
        got, st, inst = run(e, c, True)
        what = "%s %s %s best+MMTol %s" % (path, batch, "graph" if graph else "launches", form)
        check(path, st, inst, exp_best, nb, what, graph_pass=graph and form == "sized")
        same(got, best, what)
    if path in FUSED:
        kind = sc.PATHS[path][1]
        assert st["index_bytes"] == sm.index_bytes(sc.TARGETS, c, kind), (path, st["index_bytes"])


class Stream:
    """Reads of one length as the bare 2-bit stream, kept alive while the library borrows it."""

    def __init__(self, reads):
        from muscato_amd.api import concat, pack_2bit
        buf, off = concat(reads)
        packed, mask = pack_2bit(buf, int(off[-1]))
        assert mask is None
        self.n, self.L = len(reads), len(reads[0])
        self.packed = np.concatenate([packed, np.zeros(8, np.uint8)])

    def load(self, e, asyn):
        e.load_reads_packed32_ptr(self.packed.ctypes.data, 0, 0, self.L, self.n, async_upload=asyn)


@pytest.mark.parametrize("path", list(sc.PATHS))
def test_streamed_load(path):
    """A streamed load (the pass runs on the tapered batches of stream_plan, packing each as its piece arrives) against
    the blocking load of the same reads: the same counters, the plan's batch count against the uniform one."""
    from muscato_amd.api import stream_plan
    e = engine(path, batch=BATCH)
    # (MaxMatches out of the screening's reach: a pass whose screening trips is repeated with exact counters, and that
    # repeat -- whose stats the context then holds -- finds the reads resident and runs on uniform batches)
    c, reads, full, exp = sc.expected_for(path, "fixed", MaxMatches=2 ** 31 - 1)
    s = Stream(reads)
    plan = stream_plan(len(reads), 100, BATCH)
    uniform = sm.uniform_batches(len(reads), BATCH)
    assert len(plan["batch_ends"]) > uniform > 1
    for asyn, nb in ((True, len(plan["batch_ends"])), (False, uniform), (True, len(plan["batch_ends"]))):
        s.load(e, asyn)
        got, st, inst = run(e, c, False)
        what = "%s %s load" % (path, "streamed" if asyn else "blocking")
        assert not inst["exact_rerun"], what
        check(path, st, inst, exp, nb, what)
        same(got, full, what)


@pytest.mark.parametrize("path", list(sc.PATHS))
def test_first_pass_that_grows_and_repeats_a_batch(path):
    """A fresh context whose first read set is the heavy multi-map family: the first pass provides less staging /
    descriptor space than the batch needs (tests/test_stats_model.py: test_heavy_reads_outgrow_a_first_pass), grows it
    and repeats the batch.  Windows, candidates and pairs are counted once."""
    e = engine(path)
    # (MaxMatches out of the screening's reach: the exact repeat of a pass whose screening trips would replace the
    # stats of the pass that grew with those of a pass that no longer has to)
    c, reads, full, exp = sc.expected_for(path, "heavy", MaxMatches=2 ** 31 - 1)
    e.load_reads(reads)
    got, st, inst = run(e, c, False)
    assert not inst["exact_rerun"], inst
    check(path, st, inst, exp, 1, path + " heavy first pass")
    same(got, full, path)
    got, st, inst = run(e, c, False)
    check(path, st, inst, exp, 1, path + " heavy sized pass")


@pytest.mark.parametrize("batch", [None, BATCH], ids=["one-batch", "batch-1024"])
@pytest.mark.parametrize("path", list(sc.PATHS))
def test_exact_rerun_reports_one_pass(path, batch):
    """MaxMatches 40 000: enough for the pass to start with the screening sketch (its threshold, MaxMatches / (planned
    batches x workgroups), is at least 2 on the host's bound of 4096 workgroups and at most 26 on the resident grid of
    a fused kernel), and a motif read's 30 acceptances in one (window, key) block trip it: the pass runs again with
    exact block counters, which find no block near MaxMatches.  The stats are those of ONE pass."""
    e = engine(path, batch=batch)
    c, reads, full, exp = sc.expected_for(path, "ragged", MaxMatches=40000)
    e.load_reads(reads)
    nb = sm.uniform_batches(len(reads), batch) if batch else 1
    got, st, inst = run(e, c, False)
    assert inst["exact_rerun"] and inst["block_mode"] == 2, inst
    check(path, st, inst, exp, nb, path + " exact rerun")
    same(got, full, path)
    assert st["n_overflow_blocks"] == 0


@pytest.mark.parametrize("batch", [None, BATCH], ids=["one-batch", "batch-1024"])
@pytest.mark.parametrize("path", FUSED)
def test_exact_rerun_then_graph(path, batch):
    """The exact repeat and the hipGraph together (MUSC_GRAPH=1, fused paths): pass 1 of a fresh context trips the
    screening and is repeated with exact block counters, as in test_exact_rerun_reports_one_pass.  Passes 2 and 3, over
    the same reads and parameters, remember that: they start with exact counters (no repeat), find the context sized
    by the repeat, and run as a hipGraph -- the capture, then the replay (ms_screen is 0)."""
    e = engine(path, batch=batch, graph=True)
    c, reads, full, exp = sc.expected_for(path, "ragged", MaxMatches=40000)
    e.load_reads(reads)
    nb = sm.uniform_batches(len(reads), batch) if batch else 1
    for i, form in enumerate(("exact rerun", "capture", "replay")):
        got, st, inst = run(e, c, False)
        what = "%s %s %s" % (path, batch, form)
        assert inst["block_mode"] == 2 and bool(inst["exact_rerun"]) == (i == 0), (what, inst)
        check(path, st, inst, exp, nb, what, graph_pass=i > 0)
        same(got, full, what)
        assert st["n_overflow_blocks"] == 0, what


@pytest.mark.parametrize("path", list(sc.PATHS))
def test_partitions(path):
    """Three or more partitions (set_partition_bases): every counter is the sum over the partitions' passes -- each pass
    probes every read window (n_read_windows = model x partitions), finds the candidates of its own index (the model per
    partition, added), stages its own tuples -- and n_reads / n_hits are those of the merged result.  4^6 <= 2 x the
    largest partition's bases, on which the table of every partition is settled: direct, so these are equalities."""
    e = engine(path, batch=BATCH)
    e.set_partition_bases(9000)
    c, reads, full, _ = sc.expected_for(path, "ragged")
    e.load_reads(reads)
    best = best_of(full, c)
    nb = sm.uniform_batches(len(reads), BATCH)
    for apply_mmtol, tuples in ((False, full), (True, best)):
        got, st, inst = run(e, c, apply_mmtol)
        parts = e.partitions()
        npart = len(parts) - 1
        assert npart >= 3 and parts[0] == 0 and parts[-1] == len(sc.TARGETS), parts
        # (the table size is settled on the largest partition: direct for every one of them)
        assert 4 ** sc.WW <= 2 * max(sum(map(len, sc.TARGETS[a:b])) for a, b in zip(parts, parts[1:])), parts
        exp = sc.expected_for(path, "ragged", apply_mmtol=apply_mmtol, parts=parts)[3]
        assert exp["n_read_windows"] == npart * sc.expected_for(path, "ragged")[3]["n_read_windows"]
        what = "%s %d partitions%s" % (path, npart, " best+MMTol" if apply_mmtol else "")
        check(path, st, inst, exp, npart * nb, what)
        same(got, tuples, what)
        assert st["n_overflow_blocks"] == 0
        if path in FUSED:
            assert st["index_bytes"] == sm.index_bytes(sc.TARGETS, c, sc.PATHS[path][1], parts[-2], parts[-1]), what


@pytest.mark.parametrize("path", ["t2", "t4", "wide3"])
def test_reads_with_x(path):
    """X in the reads, fused path (k_match_t<.., XM = 1>): a read window that holds an X takes no part and is not
    counted; every other counter as without X."""
    e = engine(path, batch=BATCH)
    c, reads, full, exp = sc.expected_for(path, "x")
    assert exp["model"]["x_windows"] > 0
    e.load_reads(reads)
    nb = sm.uniform_batches(len(reads), BATCH)
    for form in ("careful", "sized"):
        got, st, inst = run(e, c, False)
        check(path, st, inst, exp, nb, "%s reads with X %s" % (path, form), XM=1)
        same(got, full, path)


_XDB = []


@pytest.mark.parametrize("path", ["t2", "wide3"])
def test_database_with_x(path):
    """X in the database, fused path (k_match_t<.., XM = 2>): a database window that holds an X is not indexed, so it is
    no candidate; flagged entries (one, two, several X in their context) are compared and counted like any other."""
    if not _XDB:
        _XDB.append(sc.database_with_x())
    xt = _XDB[0]
    e = engine(path, targets=xt)
    c, reads, full, exp = sc.expected_for(path, "ragged", targets=xt)
    e.load_reads(reads)
    for form in ("careful", "sized"):
        got, st, inst = run(e, c, False)
        check(path, st, inst, exp, 1, "%s database with X %s" % (path, form), XM=2)
        same(got, full, path)
    assert st["index_bytes"] == sm.index_bytes(xt, c, sc.PATHS[path][1])


@pytest.mark.parametrize("path", ["t2", "dma", "c64_2"])
def test_hashed_table(path):
    """MUSC_DEBUG_INDEX_BITS=10: 1024 buckets under a hash for 4096 keys.  Colliding keys are walked: candidates, overflow
    entries and pairs exceed the model (check(hashed=True) says why on either path); windows, accepted, hits, the launch
    counts and the fields that are zero on the path stay exact, n_descriptors <= n_pairs, and the bytes follow the
    header's formulas on the reported counts."""
    e = engine(path, extra={"MUSC_DEBUG_INDEX_BITS": "10"})
    c, reads, full, exp = sc.expected_for(path, "ragged")
    e.load_reads(reads)
    for form in ("careful", "sized"):
        got, st, inst = run(e, c, False)
        what = "%s hashed %s" % (path, form)
        check(path, st, inst, exp, 1, what, hashed=True)
        same(got, full, what)
