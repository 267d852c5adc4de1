"""The stage kernels on a grid of a few blocks (MUSC_DEBUG_STAGE_GRID), and three scan levels.

Every stage that moved onto the device is a chain of persistent kernels whose grid is capped, so that a lane or a
workgroup walks several items on a large input.  The other modules hold each stage byte for byte to its model or to the
oracle on shapes where the cap never binds: every lane makes one trip through its loop.  Here the knob takes the cap's
place -- 3 blocks (an odd stride), and 1 block once per stage (one block carries everything across its trips) -- and
the same models are held again.  The expected value always comes from the model or the oracle, never from a run of the
library; where it is cheap the case runs a second time with the knob unset and the two device outputs are compared as
well, so that a disagreement shows which side moved.

Each case asserts from its own data that the loop is crossed (`crossed`): the item count of every kernel family it
runs -- records, lines, reads, tuples, text bytes / 256, tiles, chunks, suspect blocks -- is at least three times what
a grid of 3 blocks takes in one trip: 3 x 256 lanes for the grid-stride kernels, 3 workgroups for the tile and chunk
kernels.  A case that shrinks stops passing.  Two exceptions: the cases of maxmatches_cases in test_apply_maxmatches
cross the loops over tuples and over suspect blocks only (the large case beside them crosses every loop of that stage;
the comment there says why both kinds run), and k_rebase_reads (musc_gather_rccl, a context per device) is governed by
the knob but run by no case here.

The last two tests run with the knob unset at n = 2048^2 + 1 + 2047 items = 2049 tiles: the scans' host recursion
(scan_levels) takes a third level with more than one element in it, and the second level scans 2049 sums, no multiple of
8, so that the ragged tail of scan_load8 runs (as it does at the first level of the scans over n + 1 elements) -- once
through the inclusive u32 scan (sort_unique_reads_arrays) and once through the exclusive u64 scan (prep_fastq).

Wall time on the MI355X, the models' CPU time included: the module's 43 tests 7.5 s (1.5 s of it the first Engine); the
u32 scan test 0.8 s, the u64 scan test 1.4 s; every other test under 0.5 s."""
import contextlib
import functools
import os
import random

import numpy as np
import pytest

from muscato_amd import Engine, sorted_hits
from oracle import muscato_oracle as orc

import fastq_cases as fc
import loader_cases as lc
import maxmatches_cases as mc
import read_names_cases as rn
import stats_cases as stc
import sz_cases as sc
import targets_prep_cases as tp
from cases import make_case
from test_gpu_fastq import check_against_model
from test_gpu_loaders import PROBE_TARGETS, Packed, assert_reads_resident, probe_db
from test_gpu_maxmatches import as_set, expect as mm_expect, gcfg
from test_gpu_partitions import best_of, check_read_major, raw_hits, srt, to_cfg
from test_gpu_read_names import ranked_of
from test_gpu_results import load as load_texts, oracle_text, rests_of
from test_gpu_side import TEXTS, nrecords, tails_of, text_fn
from test_cli import expected_genestats, expected_readstats

pytestmark = pytest.mark.gpu

KNOB = "MUSC_DEBUG_STAGE_GRID"
# every knob a case of this module sets, and those that would change which kernels a case runs
KNOBS = (KNOB, "MUSC_INDEX", "MUSC_CONTEXT", "MUSC_MATCH", "MUSC_SCREEN", "MUSC_GRAPH", "MUSC_BATCH_READS", "MUSC_DEBUG_MM_HEAP_LDS",
         "MUSC_DEBUG_CTX_DIRECT", "MUSC_DEBUG_INDEX_BUDGET_MB", "MUSC_DEBUG_STAGE_BYTES", "MUSC_DEBUG_STAGE_LINES")
GRID = 3          # the knob of every case
BOTH = (3, 1)     # ... and one block, once per stage
TRIPS = 3         # trips every case must give a grid of GRID blocks


@pytest.fixture(scope="module")
def eng():
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        with Engine(0) as e:
            yield e
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


@contextlib.contextmanager
def stage_grid(eng, knob, **env):
    """The calls of `eng` with MUSC_DEBUG_STAGE_GRID = knob (None: unset) and `env`; afterwards none of KNOBS is set."""
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    if knob is not None:
        os.environ[KNOB] = str(knob)
    try:
        eng.reload_env()
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
        eng.reload_env()


def crossed(what, count, per_block=256):
    """`count` items of a kernel family that takes `per_block` items per block and trip: a grid of GRID blocks makes at
    least TRIPS trips (and a grid of one block three times as many)."""
    assert count >= TRIPS * GRID * per_block, "%s: %d items give a grid of %d blocks fewer than %d trips" % (what, count, GRID, TRIPS)


def with_and_without(eng, knob, run, **env):
    """run() under the knob and with it unset -> (under the knob, unset)."""
    with stage_grid(eng, knob, **env):
        a = run()
    with stage_grid(eng, None, **env):
        b = run()
    return a, b


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and bool((a == b).all())
    return a == b


# ---------------------------------------------------------------- FASTQ to prepared reads

@functools.lru_cache(maxsize=None)
def fastq_case():
    """3 300 records: sequences of 10-80 bases, half of them drawn from a pool (groups), some with N, every fiftieth
    record with \\r\\n; MinReadLength 20 drops the short ones, MaxReadLength 60 cuts the long ones."""
    rng = random.Random(2604)
    pool = [fc.bases(rng, rng.randint(10, 80), b"ACGTTGCAN") for _ in range(900)]
    recs = []
    for i in range(3300):
        s = rng.choice(pool) if rng.random() < 0.5 else fc.bases(rng, rng.randint(10, 80))
        recs.append(fc.record(b"q%d lane:%d" % (i, i % 7), s, eol=b"\r\n" if i % 50 == 0 else b"\n"))
    return fc.Case("stage_grid", b"".join(recs), 20, 60)


@pytest.mark.parametrize("knob", BOTH)
def test_prep_fastq(eng, knob):
    c = fastq_case()

    def run():
        probe_db(eng)
        eng.load_reads([b"ACGT" * 5, b"GGGG"])
        return eng.prep_fastq(c.raw, c.min_len, c.max_len)

    out, plain = with_and_without(eng, knob, run)
    crossed("records (k_fq_records)", out["n_records"])
    crossed("kept reads (k_prep_keys, k_prep_heads, k_prep_starts)", out["n_reads"])
    crossed("records (k_fq_gather: sixteen lanes a record)", out["n_records"], 256 // 16)
    crossed("text tiles (k_fq_count, k_fq_lines)", len(c.raw) // fc.TILE, 1)
    assert out["n_short"] > 100 and out["n_unique"] < out["n_reads"] and out["max_len"] == c.max_len
    uniq = check_against_model(c, out)
    assert same(out, plain)
    with stage_grid(eng, knob):
        eng.prep_fastq(c.raw, c.min_len, c.max_len)
        assert_reads_resident(eng, uniq)


# ---------------------------------------------------------------- the read names

@functools.lru_cache(maxsize=None)
def names_raw():
    """2 400 groups of one to three reads, and four larger ones (65, 300, 700 and 1 300 members: the key passes), the
    names in reverse or scrambled file order, some with a tab, a few longer than a key word."""
    rng = random.Random(2605)
    t = rn.Text()
    for g in range(2400):
        k = 1 + g % 3
        names = [b"@s%d_%d%s" % (g, k - 1 - j, b"\tmore" if (g + j) % 5 == 0 else b"") for j in range(k)]
        t.group(names, align=g % 16 if g % 100 == 0 else None)
    for k in (65, 300, 700, 1300):
        stem = rn.long_name(rng, 11 + k % 9)
        t.group([stem + b"%05d" % ((j * 7919) % k) for j in range(k)], align=k % 16)
    return t.raw


@functools.lru_cache(maxsize=None)
def names_model():
    return rn.model(names_raw(), 1, 100)


@pytest.mark.parametrize("knob", BOTH)
def test_read_names(eng, knob):
    m = names_model()
    nu = len(m.records)
    pieces = [(0, nu), (0, 1), (nu // 2, 3), (nu - 1, 1), (7, 1000)]

    def run():
        probe_db(eng)
        eng.load_reads([b"ACGT" * 5, b"GGGG"])
        out = eng.prep_fastq_names(names_raw(), 1, 100)
        texts = [[eng.names_text(which, r0, cnt) for r0, cnt in pieces] for which in (0, 1)]
        out["names"] = {k: v for k, v in out["names"].items() if k != "ms_names"}
        return out, texts

    (out, texts), plain = with_and_without(eng, knob, run)
    info = out["names"]
    crossed("kept reads (k_rn_gid, k_rn_measure, k_rn_rank, k_rn_pairs)", out["n_reads"])
    crossed("groups (k_rn_sizes)", nu)
    crossed("members of the larger groups (k_rn_keys, k_rn_unpairs)", info["n_pairs"])
    crossed("record text bytes / 256 (k_rn_records, k_rn_copy: a wave per record)", info["text_bytes"] // 256, 1)
    crossed("groups (the renders: four waves a block)", nu, 4)
    assert m.info["n_sorted_groups"] == 4 and m.info["max_group"] == 1300
    assert out["n_unique"] == nu and out["ranked"].tolist() == ranked_of(m)
    assert (info["text_bytes"], info["line_bytes"]) == (m.info["n_text_bytes"], m.info["n_line_bytes"])
    assert (info["n_single"], info["n_counted"], info["n_sorted"]) == (m.info["n_single"], m.info["n_wave_groups"], m.info["n_sorted_groups"])
    assert info["n_pairs"] == sum(k for k in m.counts if k > rn.WAVE_GROUP_MAX) and info["key_passes"] >= 2
    for which, recs in ((0, m.records), (1, m.lines)):
        for (r0, cnt), got in zip(pieces, texts[which]):
            assert got == b"".join(recs[r0:r0 + cnt]), (which, r0, cnt)
    assert same((out, texts), plain)


# ---------------------------------------------------------------- the loaders, read back base for base

def _ragged():
    return [r for maxlen in lc.RAGGED_MAXLENS for r in lc.ragged_reads(maxlen, True)]


@pytest.mark.parametrize("knob", BOTH)
def test_ragged_read_loaders(eng, knob):
    """Host ASCII, the packed form behind 64-bit offsets, and behind 32-bit lengths (k_widen_u32 and the scan); the
    longest read comes from k_max_len, and the readback orders and renders one line per read."""
    reads = _ragged()
    crossed("reads (k_max_len; the readback's k_results_* over one tuple each)", len(reads))
    crossed("lines (k_results_render: four waves a block)", len(reads), 4)
    pk = Packed(reads)
    assert pk.nx > 0
    with stage_grid(eng, knob):
        probe_db(eng)
        eng.load_reads(reads)
        assert_reads_resident(eng, reads)
        eng.load_reads(reads[:3])
        eng.load_reads_packed_ptr(pk.b2.ctypes.data, pk.bm.ctypes.data, pk.off.ctypes.data, pk.n)
        assert_reads_resident(eng, reads)
        eng.load_reads(reads[:3])
        eng.load_reads_packed32_ptr(pk.b2.ctypes.data, pk.bm.ctypes.data, pk.lens.ctypes.data, 0, pk.n)
        assert_reads_resident(eng, reads)


def test_fixed_length_read_loader(eng):
    rng = random.Random(2606)
    L = 37
    reads = [lc.rand_bases(rng, L) for _ in range(2500)]
    crossed("reads", len(reads))
    pk = Packed(reads)
    with stage_grid(eng, GRID):
        probe_db(eng)
        eng.load_reads_packed32_ptr(pk.b2.ctypes.data, 0, 0, L, pk.n)
        assert_reads_resident(eng, reads)


@pytest.mark.parametrize("with_x", [False, True], ids=["plain", "x"])
def test_database_loaders(eng, with_x):
    """load_targets (ASCII) and load_targets_packed: every target from its first base, as many times over as it
    takes for the readback's list to cross the loops of the order and of the render."""
    targets = lc.target_set(with_x)
    rests = lc.target_rests(targets)
    read = lc.rand_bases(random.Random(300), 300)
    once = lc.target_tuples(targets)
    hits = once * (TRIPS * GRID * 256 // len(once) + 1)
    crossed("tuples (k_results_*)", len(hits))
    exp = sorted(lc.expected_lines([read], targets, rests, hits))
    with stage_grid(eng, GRID):
        for loader in (eng.load_targets, eng.load_targets_packed):
            eng.load_targets(PROBE_TARGETS)
            loader(targets)
            eng.set_gene_text(rests)
            eng.load_reads([read])
            nl, nb = eng.results_order(np.array(hits, dtype=np.uint32))
            got = eng.results_text().splitlines(True)
            assert nl == len(got) == len(exp) and nb == sum(len(x) for x in exp)
            assert sorted(got) == exp


# ---------------------------------------------------------------- snappy frames and the gene file

@functools.lru_cache(maxsize=None)
def gene_file():
    """A gene file of a little over 640 KiB: ten chunks of 65 536 bytes and a ragged eleventh.  2 900 lines
    target \\t id columns; targets of 50-400 bases, a tenth of them with an X."""
    rng = np.random.default_rng(2607)
    lines, targets = [], []
    for g in range(2900):
        t = stc.BASES[rng.integers(0, 4, size=int(rng.integers(50, 401)))].copy()
        if g % 10 == 3:
            t[int(rng.integers(0, len(t)))] = ord("X")
        targets.append(bytes(t))
        lines.append(targets[-1] + b"\t%011d\tgene%d\t%d\n" % (g, g, len(t)))
    text = b"".join(lines)
    keep = (10 * sc.MAX_CHUNK + 777)
    assert len(text) > keep
    text = text[:text.rfind(b"\n", 0, keep) + 1]
    return text, targets[:text.count(b"\n")]


PROBE_LEN = 1000
GENE_PROBE = b"ACGT" * (PROBE_LEN // 4)


def _gene_rendered(e):
    GENE_TARGETS = gene_file()[1]
    rests = lc.target_rests(GENE_TARGETS)
    hits = [(0, g, 0, 0) for g in range(len(GENE_TARGETS))]
    e.set_gene_text(rests)
    e.load_reads([GENE_PROBE])
    nl, nb = e.results_order(np.array(hits, dtype=np.uint32))
    got = e.results_text().splitlines(True)
    assert nl == len(got) == len(hits)
    return sorted(got), sorted(lc.expected_lines([GENE_PROBE], GENE_TARGETS, rests, hits))


@pytest.mark.parametrize("knob", BOTH)
def test_sz_round_trip_and_gene_file(eng, knob):
    """sz_decode of the host codec's streams, sz_frame against the host codec's uncompressed frame and back through the
    decoder, and load_db_text plain and framed: the database read back base for base."""
    text, GENE_TARGETS = gene_file()
    nch = (len(text) + sc.MAX_CHUNK - 1) // sc.MAX_CHUNK
    assert nch >= 10 and len(text) % sc.MAX_CHUNK
    crossed("chunks (k_sz_decode, k_sz_frame)", nch, 1)
    crossed("lines (k_dbt_lengths)", len(GENE_TARGETS))
    crossed("text tiles (k_fq_count, k_dbt_lines)", len(text) // fc.TILE, 1)
    comp, plain = sc.frame(text, True), sc.frame(text, False)
    assert sc.model_targets(text)[0] == GENE_TARGETS and orc.snappy_framed_decode(comp) == text
    with stage_grid(eng, knob):
        assert eng.sz_decode(comp) == text
        assert eng.sz_decode(plain) == text
        framed = eng.sz_frame(text)
        assert framed == plain
        assert eng.sz_decode(framed) == text
        for data, fr, chunks in ((text, 0, 0), (comp, 1, nch), (plain, -1, nch)):
            eng.load_targets(PROBE_TARGETS)
            info = eng.load_db_text(data, framed=fr)
            assert (info.n_targets, info.n_bases, info.n_odd, info.n_text_bytes, info.n_chunks) == \
                (len(GENE_TARGETS), sum(map(len, GENE_TARGETS)), 0, len(text), chunks)
            got, exp = _gene_rendered(eng)
            assert got == exp
    with stage_grid(eng, None):
        assert eng.sz_frame(text) == framed


# ---------------------------------------------------------------- target preparation

def _prep_records():
    rng = random.Random(2608)
    return tp._named(rng, [rng.choice((1, 3, 4, 5, 17, 40, 61, 130)) for _ in range(2400)])


@functools.lru_cache(maxsize=None)
def prep_text(fasta):
    return tp._fasta(_prep_records(), width=17) if fasta else tp._text([(n[1:], s) for n, s in _prep_records()])


@functools.lru_cache(maxsize=None)
def prep_model(fasta, rev):
    m = tp.model(prep_text(fasta), fasta, rev)
    return (m,) + tp.texts_of(m)


@pytest.mark.parametrize("fasta,rev,knob", [(True, True, 3), (True, False, 3), (False, True, 3), (False, False, 3), (True, True, 1), (False, True, 1)])
def test_prep_targets(eng, fasta, rev, knob):
    text = prep_text(fasta)
    m, seqs, ids = prep_model(fasta, rev)
    nrec = len(m.seqs) // (2 if rev else 1)
    crossed("lines (k_tp_classify, k_tp_hl)", m.n_lines)
    crossed("records (k_tp_text_recs, k_tp_groups, k_tp_compact, k_tp_idlen)", nrec)
    crossed("text tiles (k_fq_count, k_tp_lines)", len(text) // fc.TILE, 1)
    crossed("words of the two texts (k_tp_seqs, k_tp_ids)", min(len(seqs), len(ids)) // 4)
    assert m.refused is None and m.n_subx > 0
    n = len(seqs)
    ranges = ((0, 0), (0, 1), (1, n - 1), (n - 1, 1), (7, 4096), (n // 3 | 1, n // 2))

    def run():
        info = eng.prep_targets(text, fasta, rev)
        fields = (info.n_lines, info.n_records, info.n_targets, info.n_dropped, info.stop_line, info.n_subx, info.n_seq_bytes, info.n_id_bytes)
        return fields, eng.prepared_text(0), eng.prepared_text(1), [eng.prepared_text(0, off, nb) for off, nb in ranges]

    (fields, got_seqs, got_ids, parts), plain = with_and_without(eng, knob, run)
    assert fields == (m.n_lines, nrec, len(m.seqs), m.n_dropped, m.stop_line, m.n_subx, len(seqs), len(ids))
    assert got_seqs == seqs and got_ids == ids
    assert parts == [seqs[off:off + nb] for off, nb in ranges]
    assert same((fields, got_seqs, got_ids, parts), plain)


# ---------------------------------------------------------------- the index build on every kind

INDEX_KINDS = {"auto": ({}, None), "classic": ({"MUSC_INDEX": "classic"}, (0, 3)), "lines": ({"MUSC_INDEX": "lines"}, (3,)),
               "classic64": ({"MUSC_INDEX": "classic64"}, (0,)), "wide": ({"MUSC_CONTEXT": "wide"}, None)}
_index_case = []


def index_case():
    """cases.make_case(3): X in the database, three windows; its tuples by the oracle."""
    if not _index_case:
        ocfg, reads, targets = make_case(3)
        exp = np.array(sorted(orc.match_direct(reads, targets, ocfg)), dtype=np.uint32).reshape(-1, 4)
        _index_case.append((ocfg, reads, targets, exp))
    return _index_case[0]


@pytest.mark.parametrize("kind,knob", [(k, 3) for k in INDEX_KINDS] + [("auto", 1), ("classic64", 1)])
def test_index_build(eng, kind, knob):
    ocfg, reads, targets, exp = index_case()
    env, kinds = INDEX_KINDS[kind]
    nbases = sum(map(len, targets))
    crossed("chunks of 256 bases (k_index, the context-bucket build)", nbases // 256, 1)
    assert any(b"X" in t for t in targets) and len(exp) > 100

    def run():
        eng.load_targets(targets)  # (a new database: the index is built under the knob in hand)
        eng.load_reads(reads)
        got = sorted_hits(eng.match(to_cfg(ocfg), apply_mmtol=False))
        return got, eng.stats()["index_kind"]

    (got, built), plain = with_and_without(eng, knob, run, **env)
    assert kinds is None or built in kinds
    assert got.shape == exp.shape and (got == exp).all()
    assert same((got, built), plain)


# ---------------------------------------------------------------- one workload for the stages behind a pass

class Workload:
    """stats_cases' database and ragged reads (and 600 more of the same kind) with a last target of 150 bases that six reads are cut from: a partition of
    its own under the right limit, with fewer tuples than a wave has lanes.  Every accepted tuple by the literal oracle."""

    def __init__(self):
        rng = np.random.default_rng(2609)
        extra = bytes(stc.BASES[rng.integers(0, 4, size=150)])
        self.targets = list(stc.TARGETS) + [extra]
        self.reads = sorted(set(stc.read_set("ragged")) | set(stc.ragged_reads(7, 600)) | {extra[p:p + 60] for p in (0, 11, 30, 47, 71, 90)})
        self.cfg = stc.cfg((0, 20))
        self.full = stc.oracle_full(self.reads, self.targets, self.cfg)
        self.best = best_of(self.full, self.cfg.MMTol)
        self.off = np.r_[0, np.cumsum([len(t) for t in self.targets])]

    def limit(self):
        """A partition limit whose greedy cut (whole targets, at most `limit` bases from the front) ends in the last
        target alone and has at least three ranges."""
        off, n = self.off, len(self.targets)
        for lim in range(4000, 12000):
            g, cuts = 0, 0
            while g < n:
                g1 = max(int(np.searchsorted(off, off[g] + lim, side="right")) - 1, g + 1)
                cuts += 1
                if g1 == n and g == n - 1 and cuts >= 3:
                    return lim
                g = g1
        raise AssertionError("no limit leaves the last target alone")


_workload = []


def workload():
    if not _workload:
        _workload.append(Workload())
    return _workload[0]


@pytest.mark.parametrize("apply_mmtol,knob", [(False, 3), (True, 3), (True, 1)])
def test_partition_merge(eng, apply_mmtol, knob):
    w = workload()
    exp = w.best if apply_mmtol else w.full
    lim = w.limit()

    def run():
        eng.set_partition_bases(0)
        eng.load_targets(w.targets)
        eng.load_reads(w.reads)
        eng.set_partition_bases(lim)
        try:
            got = raw_hits(eng, w.cfg, apply_mmtol)
            plan = eng.partitions()
            check_read_major(eng, got)
        finally:
            eng.set_partition_bases(0)
        return got, plan

    (got, plan), plain = with_and_without(eng, knob, run)
    assert len(plan) - 1 >= 3 and plan[-2] == len(w.targets) - 1
    # what each partition's pass hands the merge: every accepted tuple of its targets, or its own best + MMTol selection
    segs = []
    for a, b in zip(plan, plan[1:]):
        part = w.full[(w.full[:, 1] >= a) & (w.full[:, 1] < b)]
        segs.append(len(best_of(part, w.cfg.MMTol)) if apply_mmtol else len(part))
    crossed("tuples of all segments (k_part_count)", sum(segs))
    assert max(segs) > 2048 and 0 < min(segs) < 64
    crossed("tuples of the longest segment (k_part_best, k_part_flags, k_part_head, k_part_scatter)", max(segs))
    crossed("tuples (k_pack_compact_range)", len(exp))
    assert srt(got).shape == exp.shape and (srt(got) == exp).all()
    # (within a read a pass emits its tuples in no fixed order: the two lists are compared sorted)
    assert same((srt(got), plan), (srt(plain[0]), plain[1]))


@pytest.mark.parametrize("knob", BOTH)
def test_packed_forms_of_a_pass(eng, knob):
    """hits_to_packed, unpack_hits (device to device) and hits_to_compact over the list of an unpartitioned pass."""
    import torch
    w = workload()
    bits = (14, 8, 12, 8)
    crossed("tuples (k_pack_hits, k_unpack_hits, k_pack_compact)", len(w.best))

    def run():
        eng.set_partition_bases(0)
        eng.load_targets(w.targets)
        eng.load_reads(w.reads)
        n = eng.match_device(to_cfg(w.cfg), apply_mmtol=True)
        host = np.zeros(n, dtype=np.uint64)
        eng.hits_to_packed(host.ctypes.data, n, False, bits, read_base=5)
        dev = torch.zeros(n, dtype=torch.int64, device="cuda")
        eng.hits_to_packed(dev.data_ptr(), n, True, bits, read_base=5)
        back = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        eng.unpack_hits(dev.data_ptr(), n, True, bits, back.data_ptr())
        torch.cuda.synchronize()
        words = torch.zeros(n, dtype=torch.int32, device="cuda")
        counts = torch.zeros(len(w.reads), dtype=torch.uint8, device="cuda")
        eng.hits_to_compact(words.data_ptr(), n, counts.data_ptr(), len(w.reads), True, (8, 12, 8))
        torch.cuda.synchronize()
        return (host, dev.cpu().numpy().view(np.uint64), back.cpu().numpy().view(np.uint32), words.cpu().numpy().view(np.uint32),
                counts.cpu().numpy())

    (host, dev, back, words, counts), plain = with_and_without(eng, knob, run)
    # (within a read a pass emits its tuples in no fixed order: the two runs' lists are compared sorted)
    assert same(np.sort(host), np.sort(plain[0])) and same(counts, plain[4])
    v = host.copy()
    dec = np.zeros((len(v), 4), dtype=np.uint32)
    for col, width in ((3, bits[3]), (2, bits[2]), (1, bits[1])):
        dec[:, col] = v & np.uint64((1 << width) - 1)
        v >>= np.uint64(width)
    dec[:, 0] = v - np.uint64(5)
    assert (srt(dec) == w.best).all() and (dev == host).all()
    back[:, 0] -= 5
    assert (back == dec).all()
    assert int(counts.sum()) == len(dec) and (np.repeat(np.arange(len(w.reads), dtype=np.uint32), counts) == dec[:, 0]).all()
    assert (np.stack([words >> 20, (words >> 8) & 0xFFF, words & 0xFF], axis=1) == dec[:, 1:]).all()


# ---------------------------------------------------------------- results.txt and the side texts

_texts = []


def workload_texts():
    """The oracle's results.txt over the oracle's tuples of the workload, and the reference tools' three side texts."""
    if not _texts:
        w = workload()
        rests = rests_of(w.targets, [b"gene_%d" % (g % 23) for g in range(len(w.targets))])
        R = [(r, 1 + i % 3, b"r%d;x%d rest" % (i // 2, i)) for i, r in enumerate(w.reads)]
        absent = (len(w.targets) - 2,)
        res = oracle_text(w.reads, w.targets, rests, w.best, tails_of(R), absent)
        ureads = [orc.UniqueRead(r, c, n) for r, c, n in R]
        side = dict(zip(TEXTS, (orc.nonmatch_text(res, ureads), expected_genestats(res), expected_readstats(res))))
        _texts.append((rests, R, absent, res, side))
    return _texts[0]


@pytest.mark.parametrize("knob", BOTH)
def test_results_and_side_texts_of_a_real_pass(eng, knob):
    w = workload()
    rests, R, absent, res, side = workload_texts()
    lines = res.splitlines(True)
    rng = random.Random(2610)
    ranges = [(0, 1), (len(lines) - 1, 1)] + [(rng.randrange(len(lines)), rng.randint(1, 3000)) for _ in range(4)]

    def run():
        eng.set_partition_bases(0)
        load_texts(eng, w.reads, w.targets, rests, tails_of(R), absent)
        n = eng.match_device(to_cfg(w.cfg), apply_mmtol=True)
        order = eng.results_order(None)
        out = {"n": n, "order": order, "text": eng.results_text(), "ranges": [eng.results_text(l0, cnt) for l0, cnt in ranges],
               "side": eng.side_prepare()}
        for which in TEXTS:
            nrec = out["side"][which][0]
            out[which] = text_fn(eng, which)()
            out[which + "_ranges"] = [text_fn(eng, which)(r0, cnt) for r0, cnt in ((0, 1), (nrec // 2, 7), (max(nrec - 40, 0), 1000))]
        return out

    out, plain = with_and_without(eng, knob, run)
    crossed("tuples (k_results_*, k_side_mark, k_side_rs_keys)", out["n"])
    crossed("lines (k_results_len; k_results_render: four waves a block)", len(lines))
    crossed("reads (k_side_tokens, k_side_nm_len, k_side_rs_flag)", len(w.reads))
    crossed("nonmatch text bytes / 256 (k_side_nm_render)", len(side["nonmatch"]) // 256, 1)
    crossed("readstats lines (k_side_rs_lines, k_side_rs_len)", side["readstats"].count(b"\n"))
    assert out["n"] == len(w.best) and out["order"] == (len(lines), len(res))
    assert out["text"] == res
    assert out["ranges"] == [b"".join(lines[l0:l0 + cnt]) for l0, cnt in ranges]
    for which in TEXTS:
        per = 4 if which == "nonmatch" else 1
        sl = side[which].splitlines(True)
        nrec = nrecords(which, side[which])
        assert out["side"][which] == (nrec, len(side[which])) and nrec > 20, which
        assert out[which] == side[which], which
        want = [b"".join(sl[per * r0:per * (r0 + cnt)]) for r0, cnt in ((0, 1), (nrec // 2, 7), (max(nrec - 40, 0), 1000))]
        assert out[which + "_ranges"] == want, which
    assert same(out, plain)


def test_side_texts_of_many_gene_names(eng):
    """2 400 short targets with a name each and a hand-fed list: the genestats kernels walk the names, which a database
    of a few dozen genes never makes them do twice."""
    rng = random.Random(2611)
    n = 2400
    targets = [lc.rand_bases(rng, 24) for _ in range(n)]
    rests = rests_of(targets, [b"name%04d" % ((g * 7) % n) for g in range(n)])
    reads = sorted({lc.rand_bases(rng, 20) for _ in range(n)})
    R = [(r, 1 + i % 4, b"t%d x" % (i // 2)) for i, r in enumerate(reads)]
    hits = [(i, (i * 13 + k) % n, k, k % 2) for i in range(len(reads)) if i % 3 for k in range(1 + i % 3)]
    crossed("gene names (k_side_gs_len, k_side_gs_render)", n)
    crossed("tuples", len(hits))
    res = oracle_text(reads, targets, rests, hits, tails_of(R))
    exp = dict(zip(TEXTS, (orc.nonmatch_text(res, [orc.UniqueRead(*x) for x in R]), expected_genestats(res), expected_readstats(res))))
    crossed("genestats lines", exp["genestats"].count(b"\n"))
    with stage_grid(eng, GRID):
        load_texts(eng, reads, targets, rests, tails_of(R))
        eng.results_order(np.array(hits, dtype=np.uint32))
        assert eng.results_text() == res
        got = eng.side_prepare()
        for which in TEXTS:
            assert text_fn(eng, which)() == exp[which], which
            assert got[which] == (nrecords(which, exp[which]), len(exp[which]))


# ---------------------------------------------------------------- the MaxMatches replay

def _mm_big_case(mode):
    """2 400 reads of 30 bases, each with 8-base keys of its own in windows 0 and 10, cut from two or three targets that
    differ from one another behind the windows: with MaxMatches 1 every read's two blocks are truncated -- 4 800 suspect
    probes in 4 800 blocks over some 6 000 tuples, so that every loop of the stage is crossed."""
    rng = np.random.default_rng(2614)
    n = 2400
    keys = rng.permutation(65536)[:2 * n]
    kmer = lambda v: bytes(stc.BASES[(int(v) >> (2 * np.arange(8))) & 3])
    reads, targets = [], []
    for i in range(n):
        r = kmer(keys[i]) + bytes(stc.BASES[rng.integers(0, 4, 2)]) + kmer(keys[n + i]) + bytes(stc.BASES[rng.integers(0, 4, 12)])
        reads.append(r)
        for copy in range(2 + i % 2):
            t = bytearray(r)
            if copy:  # a substitution behind both windows: the copies of a read's block differ in nmiss
                p = int(rng.integers(18, 30))
                t[p] = b"ACGT"[(b"ACGT".index(t[p]) + 1 + int(rng.integers(0, 3))) % 4]
            targets.append(bytes(stc.BASES[rng.integers(0, 4, 5)]) + bytes(t) + bytes(stc.BASES[rng.integers(0, 4, 5)]))
    reads = sorted(set(reads))
    random.Random(2614).shuffle(reads)
    targets = [targets[j] for j in rng.permutation(len(targets))]
    cfg = orc.Config(Windows=[0, 10], WindowWidth=8, PMatch=0.9, MinDinuc=0, MaxReadLength=30, MaxMatches=1, MMTol=1, MatchMode=mode)
    return mc.Case("big-%s-mm1" % mode, reads, targets, cfg, 2614)


@functools.lru_cache(maxsize=None)
def mm_case(name):
    if name.startswith("big-"):
        return _mm_big_case(name.split("-")[1])
    return next(c for c in mc.cases() if c.name == name)


# The big cases cross every loop of the stage, with the heap in LDS and (MUSC_DEBUG_MM_HEAP_LDS = 1, below MaxMatches + 1)
# in global memory.  The cases of maxmatches_cases are here for what the big ones lack -- heaps of 64 and 65 entries
# that sift, 16 of them in LDS -- and cross the loops over tuples and over suspect blocks only: with their 74 reads
# k_hot_probes, k_mm_heads, k_mm_blocks and k_mm_sizes make one trip there (`everything` says which case is which).
@pytest.mark.parametrize("name,lds,knob", [("big-best-mm1", None, 3), ("big-best-mm1", 1, 3), ("big-first-mm1", None, 3), ("big-best-mm1", None, 1),
                                           ("s6-w05-best-mm63", None, 3), ("s6-w05-best-mm63", 16, 3), ("s7-w036-best-mm64", None, 3),
                                           ("s6-w036-first-mm63", None, 3), ("s7-w036-best-mm64", 16, 1)])
def test_apply_maxmatches(eng, name, lds, knob):
    """The heap of k_mm_replay in LDS, and in the block's range of global memory (MUSC_DEBUG_MM_HEAP_LDS below
    MaxMatches + 1); mode first; the literal oracle's union and its best_filter."""
    case = mm_case(name)
    everything = name.startswith("big-")
    lit, best, rep = mm_expect(case)
    env = {"MUSC_DEBUG_MM_HEAP_LDS": str(lds)} if lds is not None else {}
    assert lds is None or (lds < case.cfg.MaxMatches + 1 and case.cfg.MatchMode == "best")
    assert len(rep.truncated) >= 10
    crossed("suspect blocks (k_mm_replay: a workgroup a block)", len(rep.truncated), 1)
    if everything:
        crossed("reads (k_hot_probes)", len(case.reads))
        crossed("suspect blocks (k_mm_sizes)", len(rep.truncated))

    def run():
        eng.set_partition_bases(0)
        eng.load_targets(case.targets)
        eng.load_reads(case.reads)
        out = []
        for apply_mmtol in (False, True):
            n0 = eng.match_device(gcfg(case.cfg), apply_mmtol=False)
            got = eng.apply_maxmatches(apply_mmtol)
            out.append((n0, got["truncated_blocks"], got["suspect_probes"], eng.hits()))
        return out

    out, plain = with_and_without(eng, knob, run, **env)
    for (n0, ntrunc, nsus, hits), exp in zip(out, (lit, best)):
        crossed("tuples (k_mm_pairs, k_mm_fill, k_mm_survive, k_mm_best, k_mm_compact)", n0)
        if everything:
            crossed("suspect probes (k_mm_heads, k_mm_blocks)", nsus)
        assert ntrunc == len(rep.truncated) and nsus >= ntrunc
        assert as_set(hits) == exp
    assert [(a, b, c, as_set(h)) for a, b, c, h in out] == [(a, b, c, as_set(h)) for a, b, c, h in plain]


# ---------------------------------------------------------------- three scan levels, the knob unset

# 2049 tiles: the second level scans 2049 sums in two tiles (2049 % 8 = 1: the ragged tail of scan_load8 runs there, and
# at the first level of the scans over N3 + 1 elements), the third level their two sums
N3 = 2048 * 2048 + 1 + 2047
assert (N3 + 2047) // 2048 == 2049


def test_u32_scan_of_three_levels(eng):
    """sort_unique_reads_arrays over N3 reads of 12 random bases (one key word: a single sort pass): the inclusive scan of
    the group heads has three levels, and most heads are 1, so every tile carries a sum.  Order, ustart and the group
    count against numpy.unique of the reads as numbers."""
    rng = np.random.default_rng(2612)
    n, L = N3, 12
    codes = rng.integers(0, 4, size=(n, L), dtype=np.uint8)
    R = stc.BASES[codes]
    key = np.zeros(n, dtype=np.uint64)
    for j in range(L):  # A < C < G < T as bytes and as codes: the numbers sort as the reads do
        key = key * np.uint64(4) + codes[:, j]
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    buf = np.concatenate([R.reshape(-1), np.zeros(8, np.uint8)])
    with stage_grid(eng, None):
        order, ustart = eng.sort_unique_reads_arrays(buf.ctypes.data, off.ctypes.data, n, False)
    uniq, first, counts = np.unique(key, return_index=True, return_counts=True)
    assert len(uniq) > 0.8 * n
    assert len(ustart) == len(uniq) + 1
    assert (np.diff(ustart.astype(np.int64)) == counts).all()
    assert (key[order[ustart[:-1]]] == uniq).all()          # group heads are the sorted distinct reads
    assert (order[ustart[:-1]] == first).all()               # and each group's first member is its first occurrence
    assert (key[order] == np.repeat(uniq, counts)).all()     # every member sits in its group
    assert eng.n_reads == len(uniq)


def test_u64_scan_of_three_levels(eng):
    """prep_fastq over N3 records of two widths (names of 1 and 2 bytes, sequences of 12 and 13 bases, chosen per record):
    the exclusive u64 scan of the prepared lengths, and the u32 scan of the kept flags beside it, have three levels.  The
    counts and the four span arrays against numpy's cumulative sums."""
    rng = np.random.default_rng(2613)
    n = N3
    long_name = rng.integers(0, 2, size=n, dtype=np.uint8).astype(bool)
    long_seq = rng.integers(0, 2, size=n, dtype=np.uint8).astype(bool)
    # every record as a row of the widest form, @n \n 13 bases \n + \n 13 quality bytes \n, and the bytes that stay
    rows = np.empty((n, 33), dtype=np.uint8)
    rows[:, 0], rows[:, 1], rows[:, 2] = ord("@"), ord("n"), 10
    rows[:, 3:16] = stc.BASES[rng.integers(0, 4, size=(n, 13), dtype=np.uint8)]
    rows[:, 16], rows[:, 17], rows[:, 18] = 10, ord("+"), 10
    rows[:, 19:32] = ord("I")
    rows[:, 32] = 10
    keep = np.ones((n, 33), dtype=bool)
    keep[:, 1] = long_name
    keep[:, 15] = long_seq
    keep[:, 31] = long_seq
    text = rows[keep]
    name_len = 1 + long_name.astype(np.int64)
    seq_len = 12 + long_seq.astype(np.int64)
    rec_len = name_len + 1 + seq_len + 1 + 2 + seq_len + 1
    name_off = np.cumsum(rec_len) - rec_len
    assert len(text) == int(rec_len.sum())
    with stage_grid(eng, None):
        probe_db(eng)
        out = eng.prep_fastq_device(text.ctypes.data, len(text), 1, 100, on_device=False)
    assert (out["n_records"], out["n_short"], out["n_reads"], out["max_len"]) == (n, 0, n, 13)
    assert (out["name_off"] == name_off.astype(np.uint64)).all()
    assert (out["name_len"] == name_len.astype(np.uint32)).all()
    assert (out["seq_off"] == (name_off + name_len + 1).astype(np.uint64)).all()
    assert (out["seq_len"] == seq_len.astype(np.uint32)).all()
    # the groups: the prepared reads as numbers in base 5 (a 12-base read is a prefix: it sorts in front of its extensions)
    key = np.zeros(n, dtype=np.uint64)
    for j in range(13):
        digit = (np.searchsorted(stc.BASES, rows[:, 3 + j]) + 1).astype(np.uint64)
        key = key * np.uint64(5) + (digit if j < 12 else np.where(long_seq, digit, np.uint64(0)))
    uniq, first, counts = np.unique(key, return_index=True, return_counts=True)
    order, ustart = out["order"], out["ustart"]
    assert out["n_unique"] == len(uniq) == len(ustart) - 1
    assert (np.diff(ustart.astype(np.int64)) == counts).all()
    assert (order[ustart[:-1]] == first).all()
    assert (key[order] == np.repeat(uniq, counts)).all()
