"""FASTQ parsing on the GPU (musc_reads_prep_fastq) against the pure-Python model of tests/fastq_cases.py:
counts, the four span arrays, the groups, the names joined as the reference joins them, and the reads the call leaves
loaded -- read back base for base through the results renderer and through a match.  Every comparison is
exact equality."""
import random

import numpy as np
import pytest

from muscato_amd import Config, Engine, MuscatoError, sorted_hits
from oracle import muscato_oracle as orc

import fastq_cases as fc
from cases import check_groups, mutate, rand_seq
from test_gpu_loaders import assert_reads_resident, probe_db

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in fc.cases()}
MODELS = {}


def model_of(c):
    if c.name not in MODELS:
        MODELS[c.name] = fc.model(c.raw, c.min_len, c.max_len)
    return MODELS[c.name]


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


def check_against_model(c, out):
    m = model_of(c)
    got = {k: out[k] for k in ("n_records", "n_short", "n_reads", "max_len")}
    print(c.name, got, "n_unique", out["n_unique"])
    assert got == {"n_records": m.n_records, "n_short": m.n_short, "n_reads": m.n_reads, "max_len": m.max_len}
    for k in ("name_off", "name_len", "seq_off", "seq_len"):
        assert out[k].tolist() == getattr(m, k), k
    uniq = check_groups(m.seqs, out["order"], out["ustart"])
    assert out["n_unique"] == len(uniq)
    names = [c.raw[o:o + n] for o, n in zip(out["name_off"].tolist(), out["name_len"].tolist())]
    joined = []
    for g, u in enumerate(uniq):
        grp = out["order"][out["ustart"][g]:out["ustart"][g + 1]].tolist()
        joined.append((u, len(grp), fc.join_names([names[i] for i in grp])))
    assert joined == fc.unique(m)
    return uniq


@pytest.mark.parametrize("name", sorted(CASES))
def test_prep_fastq_against_model(eng, name):
    c = CASES[name]
    probe_db(eng)
    eng.load_reads([b"ACGT" * 5, b"GGGG"])  # (so that the call does not find the records it is to make)
    out = eng.prep_fastq(c.raw, c.min_len, c.max_len)
    uniq = check_against_model(c, out)
    assert eng.n_reads == len(uniq)
    if uniq:
        assert_reads_resident(eng, uniq)
        assert eng.stats()["ms_read_prep"] > 0


def test_prep_fastq_and_prep_fastq_names_fill_one_dict(eng):
    """One converter serves both entry points: on the same text the two dicts agree on every common key, in value and in
    dtype -- with no record at all, with no kept read (every record below min_len), and with a duplicated sequence."""
    five = b"".join(fc.record(b"n%d" % i, s) for i, s in enumerate((b"ACGTACGT", b"GGGTTT", b"ACGTACGT", b"TTTTT", b"ACGTA")))
    for raw, records, kept, groups in ((b"", 0, 0, 0), (fc.record(b"s0", b"ACG") + fc.record(b"s1", b"TT"), 2, 0, 0), (five, 5, 5, 4)):
        a = eng.prep_fastq(raw, 4, 50)
        b = eng.prep_fastq_names(raw, 4, 50)
        assert (a["n_records"], a["n_reads"], a["n_unique"], eng.n_reads) == (records, kept, groups, groups)
        assert list(a) == ["n_records", "n_short", "n_reads", "n_unique", "max_len", "name_off", "seq_off", "name_len", "seq_len", "order",
                           "ustart"]
        assert list(b) == list(a) + ["ranked", "names"]
        for k, v in a.items():
            if isinstance(v, np.ndarray):
                assert v.dtype == b[k].dtype == (np.uint64 if k.endswith("_off") else np.uint32), k
                assert v.shape == b[k].shape == ((groups + 1,) if k == "ustart" else (kept,)) and (v == b[k]).all(), k
            else:
                assert type(v) is type(b[k]) is int and v == b[k], k
        assert b["ranked"].dtype == np.uint32 and sorted(b["ranked"].tolist()) == list(range(kept))


def match_case():
    rng = random.Random(31)
    targets = [rand_seq(rng, 300, b"ACGT") for _ in range(20)]
    reads = [mutate(rng, t[p:p + 70], 0.02, b"ACGTN") for t in targets for p in (0, 57, 230)]
    reads += reads[::4] + [rand_seq(rng, 15, b"ACGT"), rand_seq(rng, 70, b"acgt")]
    rng.shuffle(reads)
    raw = b"".join(fc.record(b"m%d" % i, r) for i, r in enumerate(reads))
    return orc.Config(Windows=[0, 10], WindowWidth=12, PMatch=0.95, MinDinuc=2, MaxReadLength=60, MinReadLength=20, MMTol=1), raw, targets


def test_match_after_prep_fastq(eng):
    """The tuples of a match over what prep_fastq loaded are those over load_reads of the model's distinct reads, and the
    oracle's."""
    ocfg, raw, targets = match_case()
    cfg = Config(Windows=list(ocfg.Windows), WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                 MaxReadLength=ocfg.MaxReadLength, MMTol=ocfg.MMTol)
    m = fc.model(raw, ocfg.MinReadLength, ocfg.MaxReadLength)
    uniq = sorted(set(m.seqs))
    assert m.n_short == 1 and m.n_reads > len(uniq) > 50 and any(b"X" in u for u in uniq)
    exp = np.array(sorted(orc.match_direct(uniq, targets, ocfg)), dtype=np.uint32).reshape(-1, 4)
    assert len(exp) > 40
    eng.load_targets(targets)
    out = eng.prep_fastq(raw, ocfg.MinReadLength, ocfg.MaxReadLength)
    assert out["n_unique"] == len(uniq)
    got = sorted_hits(eng.match(cfg, apply_mmtol=False))
    eng.load_reads(uniq)
    ref = sorted_hits(eng.match(cfg, apply_mmtol=False))
    assert got.shape == ref.shape == exp.shape and (got == ref).all() and (got == exp).all()


ALIGN_CASES = ("nl_16-1_k0", "nl_16+0_k1", "nl_1024-1_k1", "nl_4096+0_k3", "size_15", "size_17", "size_4097", "nl_run16",
               "dangling_2_open", "crlf", "odd_bytes", "long_read")


@pytest.mark.parametrize("shift", range(16))
def test_device_buffer_at_every_alignment(eng, shift):
    """The same texts as device buffers at base + shift.  The bytes around the text are newlines: a load that strayed
    outside it would count them."""
    import torch
    probe_db(eng)
    for name in ALIGN_CASES:
        c = CASES[name]
        n = len(c.raw)
        host = np.full(n + 48, 10, dtype=np.uint8)
        host[shift:shift + n] = np.frombuffer(c.raw, dtype=np.uint8)
        d = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        assert d.data_ptr() % 16 == 0
        out = eng.prep_fastq_device(d.data_ptr() + shift, n, c.min_len, c.max_len)
        uniq = check_against_model(c, out)
        if uniq:
            assert_reads_resident(eng, uniq)
        del d


def test_refused_calls_leave_no_reads(eng):
    """A negative MaxReadLength, and a prepared read of more than 65 535 bases (the message musc_reads_sort_unique gives):
    code 2, no reads left, and the next match returns nothing -- never the tuples of what was loaded before."""
    ocfg, raw, targets = match_case()
    cfg = Config(Windows=list(ocfg.Windows), WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                 MaxReadLength=ocfg.MaxReadLength, MMTol=ocfg.MMTol)
    long_raw = fc.record(b"ok", b"ACGT" * 10) + fc.record(b"long", b"ACGT" * 16384, qual=b"I")
    eng.load_targets(targets)
    for call, text in ((lambda: eng.prep_fastq(raw, 20, -1), r"failed \(2\).*negative"),
                       (lambda: eng.prep_fastq(long_raw, 1, 70000), r"failed \(2\).*read of 65536 bases exceeds the 65535-base record limit")):
        eng.prep_fastq(raw, ocfg.MinReadLength, ocfg.MaxReadLength)
        assert eng.n_reads > 50 and len(eng.match(cfg, apply_mmtol=False)) > 40
        with pytest.raises(MuscatoError, match=text):
            call()
        assert eng.n_reads == 0
        try:
            got = eng.match(cfg, apply_mmtol=False)
        except MuscatoError:
            continue
        assert len(got) == 0
    out = eng.prep_fastq(long_raw, 1, 65535)  # cut at the limit, the read is taken
    assert out["n_reads"] == 2 and out["max_len"] == 65535 and eng.n_reads == 2
