"""The read-name stage on the GPU (musc_reads_names_order, musc_reads_prep_fastq_names, musc_reads_names_text, DESIGN.md
23) against the pure-Python model of tests/read_names_cases.py: the ranked members of every group, the records
count\\tJ and the lines seq\\tcount\\tJ\\n, whole and in ranges, into host and device destinations at every alignment, and
what the context holds afterwards.  Every comparison is exact equality."""
import ctypes
import random

import numpy as np
import pytest

from muscato_amd import Config, Engine, MuscatoError, _lib

import read_names_cases as rn
from test_gpu_fastq import match_case
from test_gpu_loaders import probe_db

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in rn.cases()}


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


def groups_of(m):
    """What the sort + collapse leaves for the stage: the kept reads by sequence, ties in file order, and the groups."""
    by_seq = {}
    for i, s in enumerate(m.prep.seqs):
        by_seq.setdefault(s, []).append(i)
    order, ustart = [], [0]
    for s in sorted(by_seq):
        order += by_seq[s]
        ustart.append(len(order))
    return order, ustart


def ranked_of(m):
    return [y for mem in m.members for y in mem]


def larger_group(m):
    (big,) = [mem for mem in m.members if len(mem) > rn.WAVE_GROUP_MAX]
    return big


def order_of_text(eng, t, want_sorted_groups):
    m = rn.model(t.raw, 1, 100)
    assert m.info["n_sorted_groups"] == want_sorted_groups and "path:sorted" in m.cover
    order, ustart = groups_of(m)
    got = eng.names_order(t.raw, m.prep.name_off, m.prep.name_len, order, ustart)
    assert got.tolist() == ranked_of(m)
    return m


# ---- 1. the smallest shapes of the key passes
def test_names_order_smallest_shapes(eng):
    rng = random.Random(2302)
    eng.load_reads([b"ACGT" * 5, b"GGGG"])
    # two groups of 65 whose names first differ at byte d: one in reverse file order, one shuffled
    t = rn.Text()
    for i, d in enumerate((0, 7, 8, 9, 16)):
        stem = rn.long_name(rng, d + 6)
        names = [stem[:d] + bytes([48 + j]) + stem[d + 1:] for j in range(65)]
        t.group(list(reversed(names)), align=(3 * i) % 16)
        rng.shuffle(names)
        t.group(names, align=(5 * i + 1) % 16)
    m = order_of_text(eng, t, 10)
    assert all("diff:%d" % d in m.cover for d in (0, 7, 8, 9, 16)) and "reordered" in m.cover

    # a prefix with 0x00 bytes behind it: the longer name stands behind, whatever the words say
    t = rn.Text()
    special = [b"@p\0\0", b"@p" + b"\0" * 8, b"@p\0", b"@p", b"@p\0\0\0a", b"@prefix8" + b"\0" * 8, b"@prefix8", b"@prefix8\0"]
    t.group(special + [rn.long_name(rng, 12, b"@p") for _ in range(65 - len(special))], align=1)
    m = order_of_text(eng, t, 1)
    assert "prefix" in m.cover

    # equal names: file order
    t = rn.Text()
    t.group([b"@same_name_every_time"] * 70, align=9)
    m = order_of_text(eng, t, 1)
    assert larger_group(m) == sorted(larger_group(m)) and "equal" in m.cover

    # long names: a difference at byte 994 orders them, one at 995 is cut away -- a tie in file order; W = 125
    for d, cover in ((994, "diff:994"), (995, "tie_beyond:995")):
        t = rn.Text()
        stem = rn.long_name(rng, 1010)
        t.group([stem[:d] + bytes([48 + j]) + stem[d + 1:] for j in reversed(range(65))], align=d % 16)
        m = order_of_text(eng, t, 1)
        assert cover in m.cover and (larger_group(m) == sorted(larger_group(m))) == (d == 995)

    # W = 0: a larger group of empty names and nothing else to sort
    t = rn.Text()
    t.group([b"@a", b"@"], align=2)
    t.group([b""] * 65, align=4)
    order_of_text(eng, t, 1)
    assert eng.n_reads == 2  # the loaded reads are left alone


# ---- 2. the case both earlier attempts at the stage stopped at
def test_names_order_counts(eng):
    c = CASES["counts"]
    m = rn.model_of(c)
    order, ustart = groups_of(m)
    sizes = sorted(b - a for a, b in zip(ustart, ustart[1:]) if b - a > rn.WAVE_GROUP_MAX)
    assert sizes == [99, 100, 999, 1000, 1000] and sum(sizes) == 3198
    got = eng.names_order(c.raw, m.prep.name_off, m.prep.name_len, order, ustart)
    assert got.tolist() == ranked_of(m)


# ---- 3. 70 000 pairs: the radix sort leaves its single-block form
def test_names_order_fourteen_groups_of_5000(eng):
    names = [[b"@g%02d_r%04d" % (g, j) for j in reversed(range(5000))] for g in range(14)]
    flat = [n for grp in names for n in grp]
    raw = b"\n".join(flat) + b"\n"
    name_len = np.array([len(n) for n in flat], dtype=np.uint32)
    name_off = np.zeros(len(flat), dtype=np.uint64)
    name_off[1:] = np.cumsum(name_len[:-1].astype(np.uint64) + 1)
    order = np.arange(70000, dtype=np.uint32)
    ustart = np.arange(15, dtype=np.uint32) * 5000
    got = eng.names_order(raw, name_off, name_len, order, ustart)
    want = [y for g in range(14) for y in sorted(range(5000 * g, 5000 * g + 5000), key=lambda y: (flat[y], y))]
    assert want[:3] == [4999, 4998, 4997]
    assert got.tolist() == want


# ---- 4. the whole stage
def pieces(nu):
    return [(0, nu), (0, 1), (nu // 2, 3), (nu - 1, 1)] if nu else []


@pytest.mark.parametrize("name", sorted(CASES))
def test_stage_against_model(eng, name):
    import torch
    c = CASES[name]
    m = rn.model_of(c)
    nu = len(m.records)
    probe_db(eng)
    hits = np.array([(r, 0, 0, 0) for r in range(nu)], dtype=np.uint32).reshape(-1, 4)

    # what musc_reads_prep_fastq + musc_results_set_read_text leave: every loaded read with its record, one line each
    plain = eng.prep_fastq(c.raw, c.min_len, c.max_len)
    eng.set_read_text(m.records)
    assert eng.results_order(hits)[0] == nu
    want_lines = eng.results_text()

    eng.load_reads([b"ACGT" * 5, b"GGGG"])  # (so that the call does not find the records it is to make)
    out = eng.prep_fastq_names(c.raw, c.min_len, c.max_len)
    for k in ("n_records", "n_short", "n_reads", "n_unique", "max_len"):
        assert out[k] == plain[k], k
    for k in ("name_off", "name_len", "seq_off", "seq_len", "order", "ustart"):
        assert out[k].tolist() == plain[k].tolist(), k
    assert out["ranked"].tolist() == ranked_of(m)
    info = out["names"]
    print(name, info)
    assert (info["text_bytes"], info["line_bytes"]) == (m.info["n_text_bytes"], m.info["n_line_bytes"])
    assert (info["n_single"], info["n_counted"], info["n_sorted"]) == (m.info["n_single"], m.info["n_wave_groups"], m.info["n_sorted_groups"])
    assert info["n_pairs"] == sum(k for k in m.counts if k > rn.WAVE_GROUP_MAX)
    assert (info["key_passes"] >= 2) == (m.info["n_sorted_groups"] > 0) and info["key_passes"] <= 127
    assert eng.n_reads == nu
    assert eng.results_order(hits)[0] == nu
    assert eng.results_text() == want_lines  # the loaded reads and the installed read text

    texts = (m.records, m.lines)
    assert eng.names_text(0) == m.text and eng.names_text(1) == m.line_text
    for which in (0, 1):
        for r0, cnt in pieces(nu):
            want = b"".join(texts[which][r0:r0 + cnt])
            assert eng.names_text(which, r0, cnt) == want, (which, r0, cnt)
        if not nu:
            continue
        r0, cnt = pieces(nu)[2]
        want = b"".join(texts[which][r0:r0 + cnt])
        for a in range(16):  # destinations on the host and on the device at sixteen alignments, between guard bytes
            h = np.full(len(want) + 48, 0x5A, dtype=np.uint8)
            base = (16 - h.ctypes.data % 16) % 16 + a
            assert eng.names_text_into(which, r0, cnt, h.ctypes.data + base, len(want), False) == len(want)
            assert h[base:base + len(want)].tobytes() == want and set(h[:base].tolist()) <= {0x5A} and set(h[base + len(want):].tolist()) == {0x5A}
            d = torch.full((len(want) + 48,), 0x5A, dtype=torch.uint8, device="cuda")
            assert d.data_ptr() % 16 == 0
            assert eng.names_text_into(which, r0, cnt, d.data_ptr() + 16 + a, len(want), True) == len(want)
            torch.cuda.synchronize()
            g = d.cpu().numpy()
            assert g[16 + a:16 + a + len(want)].tobytes() == want and set(g[:16 + a].tolist()) == {0x5A} and set(g[16 + a + len(want):].tolist()) == {0x5A}


def test_results_text_is_identical_either_way(eng):
    """A match over what either call loaded, ordered and rendered from the resident tuples with the read text in place."""
    ocfg, raw, targets = match_case()
    cfg = Config(Windows=list(ocfg.Windows), WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                 MaxReadLength=ocfg.MaxReadLength, MMTol=ocfg.MMTol)
    m = rn.model(raw, ocfg.MinReadLength, ocfg.MaxReadLength)
    eng.load_targets(targets)
    eng.set_gene_text([b"gene%d\t%d" % (g, len(t)) for g, t in enumerate(targets)])
    texts = []
    for names_on_device in (False, True):
        if names_on_device:
            eng.prep_fastq_names(raw, ocfg.MinReadLength, ocfg.MaxReadLength)
        else:
            eng.prep_fastq(raw, ocfg.MinReadLength, ocfg.MaxReadLength)
            eng.set_read_text(m.records)
        assert len(eng.match(cfg)) > 40
        nl, nb = eng.results_order()
        texts.append(eng.results_text())
        assert nl > 40 and len(texts[-1]) == nb
    assert texts[0] == texts[1]
    assert all(ln.split(b"\t", 6)[6] + b"\n" in {r + b"\n" for r in m.records} for ln in texts[1].split(b"\n")[:-1])


# ---- 5. refused calls, and what the context holds afterwards
def test_refused_calls(eng):
    lib, h = eng._lib, eng._h
    c = CASES["group_sizes"]
    m = rn.model_of(c)
    order, ustart = groups_of(m)
    n, nu = len(order), len(ustart) - 1
    buf = np.frombuffer(c.raw, dtype=np.uint8)
    no = np.array(m.prep.name_off, dtype=np.uint64)
    nl = np.array(m.prep.name_len, dtype=np.uint32)
    od = np.array(order, dtype=np.uint32)
    us = np.array(ustart, dtype=np.uint32)
    ranked = np.zeros(n, dtype=np.uint32)
    good = eng.prep_fastq_names(c.raw, c.min_len, c.max_len)
    lines = eng.names_text(1)
    assert good["n_unique"] == nu == eng.n_reads and lines == m.line_text

    def order_call(text=buf.ctypes.data, nbytes=len(buf), name_off=no, name_len=nl, count=n, members=od, starts=us, groups=nu, dst=ranked):
        return lib.musc_reads_names_order(h, text, nbytes, 0, name_off.ctypes.data if name_off is not None else None,
                                          name_len.ctypes.data if name_len is not None else None, count,
                                          members.ctypes.data if members is not None else None, starts.ctypes.data if starts is not None else None,
                                          groups, dst.ctypes.data if dst is not None else None)

    assert order_call() == 0 and ranked.tolist() == ranked_of(m)
    bad_member, bad_off, bad_len, bad_start, empty_group = od.copy(), no.copy(), nl.copy(), us.copy(), us.copy()
    bad_member[3] = n
    bad_off[5] = len(buf) + 1
    bad_len[n - 1] = len(buf)
    bad_start[nu] = n - 1
    empty_group[2] = empty_group[1]
    for kw in (dict(count=0xFFFFFFF0), dict(count=1 << 40), dict(text=None), dict(name_off=None), dict(name_len=None), dict(members=None),
               dict(starts=None), dict(dst=None), dict(members=bad_member), dict(name_off=bad_off), dict(name_len=bad_len),
               dict(starts=bad_start), dict(starts=empty_group), dict(groups=n + 1), dict(groups=nu - 1)):
        assert order_call(**kw) == 2, kw
        assert len(lib.musc_last_error(h)) > 0
    # ... which leave the context's reads and texts alone
    assert eng.n_reads == nu and eng.names_text(1) == lines

    nb = ctypes.c_uint64(7)
    for args in ((2, 0, 1, None, 0, 0, ctypes.byref(nb)), (-1, 0, 1, None, 0, 0, ctypes.byref(nb)), (0, 0, 1, None, 0, 0, None)):
        assert lib.musc_reads_names_text(h, *args) == 2
    one = np.zeros(len(m.records[0]), dtype=np.uint8)
    assert lib.musc_reads_names_text(h, 0, 0, 1, one.ctypes.data, len(one) - 1, 0, ctypes.byref(nb)) == 2 and nb.value == 0  # capacity one short
    assert eng.names_text(0, nu, 5) == b"" and eng.names_text(0, 0, 0) == b""

    # a refused load: no reads, no read text, nothing to render
    fp, info = _lib.MuscFastqPrep(), _lib.MuscReadNames()
    assert lib.musc_reads_prep_fastq_names(h, buf.ctypes.data, len(buf), 0, 1, 100, None, ctypes.byref(info)) == 2
    assert lib.musc_reads_prep_fastq_names(h, buf.ctypes.data, len(buf), 0, 1, 100, ctypes.byref(fp), None) == 2
    assert lib.musc_reads_prep_fastq_names(h, None, len(buf), 0, 1, 100, ctypes.byref(fp), ctypes.byref(info)) == 2
    assert eng.names_text(1) == lines  # (refused before anything changed)
    with pytest.raises(MuscatoError, match=r"failed \(2\).*negative"):
        eng.prep_fastq_names(c.raw, 1, -1)
    assert eng.n_reads == 0
    with pytest.raises(MuscatoError, match=r"failed \(2\).*no read names rendered"):
        eng.names_text(1)
    long_raw = b"@ok\n" + b"ACGT" * 10 + b"\n+\n" + b"I" * 40 + b"\n@long\n" + b"ACGT" * 16384 + b"\n+\nI\n"
    eng.prep_fastq_names(c.raw, c.min_len, c.max_len)
    with pytest.raises(MuscatoError, match=r"failed \(2\).*65536 bases"):
        eng.prep_fastq_names(long_raw, 1, 70000)
    assert eng.n_reads == 0
    with pytest.raises(MuscatoError, match=r"failed \(2\)"):
        eng.names_text(0)

    # the texts go with the reads and with the read text they belong to
    probe_db(eng)
    eng.prep_fastq_names(c.raw, c.min_len, c.max_len)
    assert eng.names_text(1) == lines
    eng.set_read_text(m.records)
    with pytest.raises(MuscatoError, match=r"failed \(2\).*no read names rendered"):
        eng.names_text(0)
    eng.prep_fastq_names(c.raw, c.min_len, c.max_len)
    eng.prep_fastq(c.raw, c.min_len, c.max_len)
    with pytest.raises(MuscatoError, match=r"failed \(2\).*no read names rendered"):
        eng.names_text(1)
    assert eng.prep_fastq_names(b"", 1, 100)["n_unique"] == 0 and eng.names_text(1) == b"" and eng.names_text(0) == b""
