"""One context, a long life: seeded random walks over the C ABI (tests/walk_cases.py), every result held to the CPU oracle
for the inputs and parameters in hand at that step -- never to another GPU path or to a fresh engine.

Each test makes one Engine and keeps it for the whole walk: loads through every loader, index builds ahead of the pass,
partition limits, musc_reload_env after a knob flipped, passes downloaded in every wire format and repeated (sized, then
graph replay where MUSC_GRAPH is on), the MaxMatches replay, the results and side stages over random ranges.  After every
pass the path that ran (index kind, kernel instance, partitions) is asserted FIRST against the class the model expects,
then the tuples and the counts.  Every message carries the walk, the step and the steps so far;
walk_cases.replay(seed, upto) rebuilds them.

An error the model did not predict (a HIP failure, code 10, among them) is a finding: the walk stops there and raises,
and the walks after it in this module are skipped, so that nothing more of it starts on the device.

PINNED holds the shortest step lists that once failed, by name.  The first three are what the first run of this module
found: a partitioned pass over few reads returned one tuple too many, a duplicate or an unwritten slot (the merge's
per-wave run reduction took two runs of one read, from two partitions' segments within 64 tuples, for one run:
kernels_partition.hpp).  The fourth: musc_match* on a context that never had a read load answered 12, "internal"."""
import os
import re

import numpy as np
import pytest

from muscato_amd import Config, Engine, MuscatoError
from muscato_amd.api import concat, pack_2bit

import cases
import walk_cases as wc

pytestmark = pytest.mark.gpu

TROUBLE = []  # the first unpredicted error of the module: the walks after it do not start
PACKED_BITS = (16, 16, 16, 16)
COMPACT_BITS = (8, 12, 8)  # gene | pos | nmiss: 40 targets of at most 300 bases
PINNED = {  # name -> (steps, MUSC_BATCH_READS=64 at musc_init)
    "partitions, short segments": ([("db", "ragged", "packed"), ("reads", "r100b", "sort_unique"), ("part", 1),
                                    ("pass", "win5", False, "packed", 1)], False),
    "partitions, short segments, best + MMTol": ([("db", "xdb", "ascii"), ("part", 1), ("reads", "r100b", "fastq"),
                                                  ("pass", "p0", True, "dev", 1)], False),
    "partitions, short segments, two kernels": ([("db", "plain", "ascii"), ("part", 1), ("reads", "r250", "sort_unique"),
                                                 ("pass", "ww12", False, "packed", 1)], True),
    "a pass before any read load": ([("db", "plain", "ascii"), ("pass", "p0", False, "dev", 1), ("reads", "one", "ascii"),
                                     ("pass", "p0", False, "dev", 1)], False),
}


class Unpredicted(Exception):
    pass


def gcfg(par):
    o = wc.params_of(par)
    return Config(Windows=list(o.Windows), WindowWidth=o.WindowWidth, PMatch=o.PMatch, MinDinuc=o.MinDinuc,
                  MaxReadLength=o.MaxReadLength, MaxMatches=o.MaxMatches, MMTol=o.MMTol, MatchMode=o.MatchMode)


def call(fn, error):
    """fn(), which must fail with the code and text of `error` when the model says so; -> (failed, result)."""
    try:
        out = fn()
    except MuscatoError as e:
        if error is None:
            raise Unpredicted("an error the model did not predict: %s" % e)
        assert "(%d)" % error[0] in str(e) and re.search(error[1], str(e)), "refused with %r, expected %r" % (str(e), error)
        return True, None
    assert error is None, "succeeded, expected the refusal %r" % (error,)
    return False, out


def as_tuples(a):
    t = [tuple(int(v) for v in row) for row in a]
    assert all(x[0] <= y[0] for x, y in zip(t, t[1:])), "the list is not read-major"
    assert len(set(t)) == len(t), "a tuple twice"
    return tuple(sorted(t))


def load_reads(eng, name, loader, salt, keep):
    reads = wc.reads_of(name)
    if loader == "ascii":
        eng.load_reads(reads)
    elif loader == "packed":
        eng.load_reads_packed(reads)
    elif loader in ("packed32", "stream"):
        buf, off = concat(reads)
        packed, mask = pack_2bit(buf, int(off[-1]))
        packed = np.concatenate([packed, np.zeros(8, np.uint8)])
        keep[:] = [packed, mask]  # (a streamed load borrows the buffer until the pass)
        if loader == "stream":
            assert mask is None and {len(r) for r in reads} == {wc.FIXED_LEN[name]}
            eng.load_reads_packed32_ptr(packed.ctypes.data, 0, 0, wc.FIXED_LEN[name], len(reads), async_upload=True)
        else:
            lens = np.array([len(r) for r in reads], dtype=np.uint32)
            eng.load_reads_packed32_ptr(packed.ctypes.data, mask.ctypes.data if mask is not None else 0, lens.ctypes.data, 0, len(reads))
    elif loader == "sort_unique":
        raw = wc.raw_reads(name, salt)
        order, ustart = eng.sort_unique_reads(raw)
        assert cases.check_groups(raw, order, ustart) == reads
    elif loader == "fastq":
        out = eng.prep_fastq(wc.fastq_of(name, salt), 0, 1000)
        assert (out["n_unique"], out["n_short"]) == (len(reads), 0)
    else:
        raise ValueError(loader)


def download(eng, cfg, apply_mmtol, how, nreads):
    """One pass, its list in the wire format `how`, decoded -> uint32 [n, 4]."""
    if how == "host":
        return eng.match(cfg, apply_mmtol=apply_mmtol)
    n = eng.match_device(cfg, apply_mmtol=apply_mmtol)
    out = np.zeros((n, 4), dtype=np.uint32)
    if how == "dev":
        if n:
            eng.hits_to(out.ctypes.data, n, False)
    elif how == "packed":
        if n:
            words = np.zeros(n, dtype=np.uint64)
            eng.hits_to_packed(words.ctypes.data, n, False, PACKED_BITS)
            eng.unpack_hits(words.ctypes.data, n, False, PACKED_BITS, out.ctypes.data)
    else:
        words = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
        counts = np.full(max(nreads, 1), 0xFF, dtype=np.uint8)
        eng.hits_to_compact(words.ctypes.data, n, counts.ctypes.data, nreads, False, COMPACT_BITS)
        words, counts = words[:n], counts[:nreads]
        assert int(counts.sum()) == n
        g, p, x = COMPACT_BITS
        out = np.stack([np.repeat(np.arange(nreads, dtype=np.uint32), counts), words >> (p + x), (words >> x) & ((1 << p) - 1),
                        words & ((1 << x) - 1)], axis=1).astype(np.uint32).reshape(-1, 4)
    return out


def check_path(eng, par, path, nreads):
    """Which index, kernel instance and partitions the pass just run took, against the model's class."""
    st, li = eng.stats(), eng.last_instance()
    assert eng.partitions() == path["first"], "partitions %r, expected %r" % (eng.partitions(), path["first"])
    if not nreads:
        return st
    assert st["index_kind"] == path["kind"], "index kind %d, expected %r" % (st["index_kind"], path)
    W = min(len(wc.params_of(par).Windows), 4)
    if path["kind"] in (1, 2):
        d = li["match"]
        assert li["path"] == "fused" and d["kernel"] == path["family"] and d["RW"] == path["RW"], (li, path)
        if d["kernel"] == "k_match_t":
            assert (d["W"], d["XM"], d["WIDE"], d["SG"]) == (W, path["XM"], path["WIDE"], 0), (li, path)
    else:
        d = li["screen"]
        assert li["path"] == "two-kernel" and d["kernel"] == path["family"] and d["RW"] == path["RW"], (li, path)
        if d["kernel"] == "k_screen":
            assert (d["one"], d["lines"]) == (int(W <= 2), int(path["kind"] == 3)), (li, path)
        if li["confirm"] is not None:
            assert (li["confirm"]["RW"], li["confirm"]["mask"], li["confirm"]["w2"]) == (path["RW"], path["mask"], int(W <= 2)), (li, path)
    return st


def do_step(eng, m, step, exp, salt, keep, tally):
    k = step[0]
    if k == "db":
        (eng.load_targets if step[2] == "ascii" else eng.load_targets_packed)(wc.db_of(step[1]))
    elif k == "reads":
        load_reads(eng, step[1], step[2], salt, keep)
    elif k == "bad_reads":
        buf, off = concat(wc.reads_of("r100"))
        off[0] = 1
        call(lambda: eng.load_reads_arrays(buf, off), exp["error"])
    elif k == "index":
        if "first" in exp:
            eng.build_index_for(gcfg(step[1]), max(1, max([len(r) for r in wc.reads_of(m.reads)], default=0)))
            assert eng.partitions() == exp["first"]
    elif k == "part":
        eng.set_partition_bases(wc.PART_BASES if step[1] else 0)
    elif k == "env":
        if step[2] is None:
            os.environ.pop(step[1], None)
        else:
            os.environ[step[1]] = step[2]
        eng.reload_env()
    elif k == "pass":
        _, par, apply_mmtol, how, times = step
        cfg = gcfg(par)
        if exp["error"]:
            call(lambda: eng.match_device(cfg, apply_mmtol=apply_mmtol), exp["error"])
            return
        _, db, reads, _, _ = exp["list"]
        nreads = len(wc.reads_of(reads))
        want = wc.pass_tuples(db, reads, par, apply_mmtol)
        for t in range(times):
            _, got = call(lambda: download(eng, cfg, apply_mmtol, how, nreads), None)
            st = check_path(eng, par, exp["path"], nreads)
            got = as_tuples(got)
            assert got == want, "pass %d of %d: %d tuples, the oracle has %d; first difference %r" % (
                t + 1, times, len(got), len(want), sorted(set(got) ^ set(want))[:3])
            assert (st["n_hits"], st["n_accepted"], st["n_reads"]) == (len(want), len(wc.full_tuples(db, reads, par)), nreads)
            if wc.hot(db, reads, par):
                assert 1 <= st["n_overflow_blocks"] < 2 ** 64 - 1, "blocks above MaxMatches, and no verdict"
            if tally is not None:
                li = eng.last_instance()
                tally[exp["path"]["cls"]] = tally.get(exp["path"]["cls"], 0) + 1
                tally["exact rerun"] = tally.get("exact rerun", 0) + li["exact_rerun"]
                tally["batches > 1"] = tally.get("batches > 1", 0) + (st["n_batches"] > 1)
    elif k == "replay":
        failed, got = call(lambda: eng.apply_maxmatches(step[1]), exp["error"])
        if not failed:
            want = wc.list_tuples(exp["list"])
            assert got["truncated_blocks"] == exp["truncated"] <= got["suspect_probes"], (got, exp["truncated"])
            assert got["nhits"] == eng.stats()["n_hits"] == len(want), (got, len(want))
            assert as_tuples(eng.hits()) == want
    elif k == "probes":
        if exp["list"]:
            st = eng.stats()
            hot = wc.hot(*exp["list"][1:4])
            if st["n_overflow_blocks"] not in (0, 2 ** 64 - 1):
                assert hot <= set(map(tuple, eng.overflow_probes().tolist()))
            else:
                assert not hot
    elif k == "gtext":
        eng.set_gene_text(wc.gene_rests(m.db))
    elif k == "rtext":
        if not exp.get("skip"):
            eng.set_read_text(wc.read_tails(m.reads))
    elif k == "order":
        failed, got = call(lambda: eng.results_order(None), exp["error"])
        if not failed:
            lines = wc.ordered_lines(*exp["lines"])
            assert got == (len(lines), sum(map(len, lines)))
    elif k == "rhits":
        failed, got = call(eng.results_hits, exp["error"])
        if not failed:
            from test_gpu_results import six_of
            key, _ = exp["lines"]
            args = (wc.reads_of(key[2]), wc.db_of(key[1]), wc.gene_rests(key[1]))
            assert [six_of(*args, h) for h in got] == sorted(six_of(*args, h) for h in wc.list_tuples(key))
    elif k == "text":
        lines = wc.ordered_lines(*exp["lines"]) if not exp["error"] else ()
        l0 = step[1] % (len(lines) + 1)
        failed, got = call(lambda: eng.results_text(l0, step[2]), exp["error"])
        if not failed:
            assert got == b"".join(lines[l0:l0 + step[2]])
    elif k == "side":
        failed, got = call(eng.side_prepare, exp["error"])
        if not failed:
            for w, text in enumerate(wc.side_texts(exp["side"])):
                assert got[wc.SIDE[w]] == (len(wc.side_records(w, text)), len(text)), wc.SIDE[w]
    elif k == "side_text":
        recs = wc.side_records(step[1], wc.side_texts(exp["side"])[step[1]]) if not exp["error"] else []
        r0 = step[2] % (len(recs) + 1)
        failed, got = call(lambda: getattr(eng, wc.SIDE[step[1]] + "_text")(r0, step[3]), exp["error"])
        if not failed:
            assert got == b"".join(recs[r0:r0 + step[3]])
    else:
        raise ValueError(step)


def run_walk(steps, label, batch64=False, tally=None):
    """Drive one fresh Engine through `steps`; the environment is put back whatever happens."""
    old = {k: os.environ.pop(k, None) for k in wc.KNOBS}
    if batch64:
        os.environ["MUSC_BATCH_READS"] = "64"
    m = wc.Model(batch64)
    keep = []
    try:
        with Engine(0) as eng:
            for i, step in enumerate(steps):
                exp = m.apply(step)
                try:
                    do_step(eng, m, step, exp, i, keep, tally)
                except (AssertionError, Unpredicted, MuscatoError) as e:
                    msg = "%s\nwalk %s, step %d %r; the steps so far:\n%r" % (e, label, i, step, steps[:i + 1])
                    if isinstance(e, AssertionError):
                        raise AssertionError(msg) from None
                    TROUBLE.append(msg)
                    raise Unpredicted(msg) from None
    finally:
        for k in wc.KNOBS:
            os.environ.pop(k, None)
        for k, v in old.items():
            if v is not None:
                os.environ[k] = v


def guarded(steps, label, batch64=False):
    if TROUBLE:
        pytest.skip("an earlier walk of this module met an error the model did not predict")
    run_walk(steps, label, batch64)


@pytest.mark.parametrize("walk", ["seed %d" % s for s in wc.SEEDS] + sorted(PINNED))
def test_walk(walk):
    if walk in PINNED:
        guarded(PINNED[walk][0], walk, PINNED[walk][1])
    else:
        seed = int(walk.split()[1])
        guarded(wc.generate(seed), walk, wc.batch64_of(seed))


def test_every_ordered_pair_of_path_classes():
    guarded(wc.directed(), "directed")
