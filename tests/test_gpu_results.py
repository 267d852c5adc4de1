"""results.txt ordered and rendered on the device (musc_results_*) against the oracle's post-chain.

The expected bytes are always oracle.muscato_oracle.results_text over the fed tuples, with MMTol large enough to keep
every one of them; the tail of a line (count and names) is whatever text the test gave the read, so the oracle's own
two last columns are replaced by it.  The tuple lists are fed by hand, so no matching workload is needed -- but for the
last test, which orders the list a real pass left on the device."""
import contextlib
import ctypes
import os
import random

import numpy as np
import pytest

from muscato_amd import Config, Engine, MuscatoError
from oracle import muscato_oracle as orc

from cases import make_case, mutate, rand_seq

pytestmark = pytest.mark.gpu

KEEP_ALL = 1 << 30


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


def six_of(reads, targets, rests, h):
    r, g, p, nx = (int(v) for v in h)
    return b"\t".join([reads[r], targets[g][p:p + len(reads[r])], b"%d" % p, b"%d" % nx, rests[g]])


def oracle_text(reads, targets, rests, hits, tails=None, absent=()):
    ids = [b"%011d\t%s" % (g, rests[g]) for g in range(len(targets))]
    ureads = [orc.UniqueRead(r, 1, b"n") for r in reads]
    kept = [tuple(int(v) for v in h) for h in hits if int(h[1]) not in absent]
    txt = orc.results_text(kept, ureads, targets, ids, orc.Config(MMTol=KEEP_ALL))
    tail_of = dict(zip(reads, tails)) if tails is not None else None
    out = []
    for ln in txt.split(b"\n")[:-1]:
        six = ln.rsplit(b"\t", 2)[0]
        out.append(six + (b"\t" + tail_of[six.split(b"\t", 1)[0]] if tail_of is not None else b"") + b"\n")
    return b"".join(out)


def rests_of(targets, names):
    return [b"%s\t%d" % (n, len(t)) for n, t in zip(names, targets)]


def load(eng, reads, targets, rests, tails=None, absent=()):
    assert reads == sorted(set(reads))
    eng.load_targets(targets)
    eng.load_reads(reads)
    eng.set_gene_text(rests, [g in absent for g in range(len(targets))] if absent else None)
    if tails is not None:
        eng.set_read_text(tails)


def check(eng, reads, targets, rests, hits, tails=None, absent=()):
    """Order `hits` (a host list) and compare count, bytes and tuple order with the oracle."""
    exp = oracle_text(reads, targets, rests, hits, tails, absent)
    nl, nb = eng.results_order(np.array(hits, dtype=np.uint32).reshape(-1, 4))
    assert (nl, nb) == (exp.count(b"\n"), len(exp))
    got = eng.results_text()
    assert got == exp
    sixes = [six_of(reads, targets, rests, h) for h in eng.results_hits()]
    assert sixes == sorted(six_of(reads, targets, rests, h) for h in hits if int(h[1]) not in absent)
    return exp


def test_number_text(eng):
    reads = [b"A" * 30]
    targets = [b"A" * 2000, b"A" * 2000]
    rests = rests_of(targets, [b"g", b"g"])  # two byte-identical genes
    hits = [(0, 0, p, 0) for p in (2, 9, 10, 99, 100, 1000)] + [(0, 0, 5, 9), (0, 1, 5, 10), (0, 1, 10, 0)]
    load(eng, reads, targets, rests, [b"3\tr1;r2;r3"])
    exp = check(eng, reads, targets, rests, hits, [b"3\tr1;r2;r3"])
    pos = [int(ln.split(b"\t")[2]) for ln in exp.split(b"\n")[:-1]]
    assert pos == [10, 10, 100, 1000, 2, 5, 5, 9, 99]  # "10" < "9", "5\t10" < "5\t9"


def test_gene_tie_break_and_absent_gene(eng):
    reads = [b"ACGTACGTAC"]
    t = b"TTACGTACGTACTT"
    targets = [t] * 5
    rests = rests_of(targets, [b"g1", b"g10", b"g9", b"g1", b"gone"])
    hits = [(0, g, 2, 0) for g in (4, 2, 1, 0, 3)]
    load(eng, reads, targets, rests, [b"1\tr"], absent=(4,))
    exp = check(eng, reads, targets, rests, hits, [b"1\tr"], absent=(4,))
    assert exp.count(b"\n") == 4 and b"gone" not in exp
    assert [ln.split(b"\t")[4] for ln in exp.split(b"\n")[:-1]] == [b"g1", b"g1", b"g10", b"g9"]


def test_one_read_of_two_tuples(eng):
    """The smallest list that goes through the key passes: one read, two tuples that tie up to the gene text, handed
    over in line order and reversed."""
    reads = [b"ACGTACGTAC"]
    targets = [b"TTACGTACGTACTT", b"GGACGTACGTACGG"]
    rests = rests_of(targets, [b"g2", b"g1"])
    load(eng, reads, targets, rests, [b"1\tr"])
    for hits in ([(0, 1, 2, 0), (0, 0, 2, 0)], [(0, 0, 2, 0), (0, 1, 2, 0)]):
        exp = check(eng, reads, targets, rests, hits, [b"1\tr"])
        assert [ln.split(b"\t")[4] for ln in exp.split(b"\n")[:-1]] == [b"g1", b"g2"]


LENS = [1, 20, 21, 22, 42, 43, 63, 64, 100, 253, 300]


def test_span_phases(eng):
    """Targets back to back at odd lengths, so that spans start at every phase of a 16-base word and cross u32, u64 and
    target boundaries; for each read length a pair of targets whose spans differ in their last base only."""
    rng = random.Random(2)
    reads = sorted({rand_seq(rng, L, b"ACGT") for L in LENS}, key=lambda r: r)
    assert sorted(len(r) for r in reads) == LENS
    A = rand_seq(rng, 347, b"ACGT")
    P = 20
    targets = [rand_seq(rng, 5, b"ACGT"), A, rand_seq(rng, 3, b"ACGT")]
    twin = {}
    for L in LENS:
        b = bytearray(A)
        b[P + L - 1] = b"CGTA"[b"ACGT".index(A[P + L - 1])]
        twin[L] = len(targets)
        targets.append(bytes(b))
    rests = rests_of(targets, [b"t%d" % g for g in range(len(targets))])
    hits = []
    for i, r in enumerate(reads):
        L = len(r)
        hits += [(i, 1, p, p % 3) for p in range(18)]
        hits += [(i, 1, P, 1), (i, twin[L], P, 1)]
        hits += [(i, 1, 347 - L // 2, 0), (i, 3, 347 - 1, 2), (i, 2, 1, 0)]  # clipped at the target's end
    tails = [b"%d\tn%d" % (i + 1, i) for i in range(len(reads))]
    load(eng, reads, targets, rests, tails)
    check(eng, reads, targets, rests, hits, tails)


@pytest.mark.parametrize("read_x,db_x", [(True, True), (True, False), (False, True), (False, False)])
def test_x_in_reads_and_targets(eng, read_x, db_x):
    core = b"ACGTTACGTACGGATTACAGATTACAGG"
    reads = sorted([core, core[:4] + b"X" + core[5:]] if read_x else [core, core[:-1] + b"A"])
    t0 = b"GG" + core + b"TT"
    targets = [t0, t0[:6] + (b"X" if db_x else b"G") + t0[7:], t0[:-3] + b"TTT", b"CC" + core[:20]]
    # targets 0 and 1 differ at span base 4: T against X (or G) decides; target 2 differs in the span's last base
    rests = rests_of(targets, [b"a", b"a", b"a", b"b"])
    hits = [(r, g, 2, r) for r in range(2) for g in range(3)] + [(1, 3, 2, 0), (0, 3, 0, 4)]
    load(eng, reads, targets, rests, [b"1\tx", b"2\ty;z"])
    exp = check(eng, reads, targets, rests, hits, [b"1\tx", b"2\ty;z"])
    assert (b"X" in exp) == (read_x or db_x)
    if db_x:
        subs = [ln.split(b"\t")[1] for ln in exp.split(b"\n")[:-1] if ln.startswith(reads[0] + b"\t") and len(ln.split(b"\t")[1]) == len(core)]
        assert subs.index(t0[2:2 + len(core)]) < subs.index(targets[1][2:2 + len(core)])  # ...T... before ...X...


def test_clipping_and_bad_positions(eng):
    rng = random.Random(4)
    reads = [rand_seq(rng, 30, b"ACGT")]
    targets = [rand_seq(rng, 50, b"ACGT"), rand_seq(rng, 17, b"ACGT")]
    rests = rests_of(targets, [b"u", b"v"])
    good = [(0, 0, 40, 3), (0, 0, 50, 30), (0, 0, 20, 0), (0, 1, 17, 1), (0, 1, 0, 2)]
    load(eng, reads, targets, rests, [b"1\tr"])
    exp = check(eng, reads, targets, rests, good, [b"1\tr"])
    assert reads[0] + b"\t\t50\t30\tu\t50\t1\tr\n" in exp  # pos == the target's length: an empty targetsub
    for bad in [(0, 0, 51, 0), (0, 1, 18, 0), (1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 4294967295, 0)]:
        with pytest.raises(MuscatoError, match="outside the loaded reads and targets"):
            eng.results_order(np.array(good + [bad], dtype=np.uint32))
        with pytest.raises(MuscatoError):
            eng.results_text()  # a failed order leaves no list behind
    # the same through a device list: the flagging kernel refuses it before any dependent load
    import torch
    nl, nb = ctypes.c_uint64(), ctypes.c_uint64()
    for lst, rc_exp in [(good + [(0, 0, 51, 0)], 2), (good + [(7, 0, 0, 0)], 2), (good + [(0, 9, 0, 0)], 2), (good, 0)]:
        d = torch.from_numpy(np.array(lst, dtype=np.uint32).view(np.int32)).cuda()
        rc = eng._lib.musc_results_order(eng._h, d.data_ptr(), len(lst), 1, ctypes.byref(nl), ctypes.byref(nb))
        assert rc == rc_exp, eng._lib.musc_last_error(eng._h)
    assert (nl.value, nb.value) == (len(good), len(exp))
    assert eng.results_text() == exp


def test_read_that_is_a_prefix_of_the_next(eng):
    t = b"GGACGTACGTACGGTT"
    reads = [b"ACGTACGTAC", b"ACGTACGTACGG"]
    targets = [t, t]
    rests = rests_of(targets, [b"p", b"q"])
    hits = [(1, 0, 2, 0), (0, 0, 2, 0), (1, 1, 2, 0), (0, 1, 2, 0)]
    load(eng, reads, targets, rests, [b"1\ta", b"1\tb"])
    exp = check(eng, reads, targets, rests, hits, [b"1\ta", b"1\tb"])
    assert [ln.split(b"\t")[0] for ln in exp.split(b"\n")[:-1]] == [reads[0]] * 2 + [reads[1]] * 2


@pytest.fixture(scope="module")
def segments():
    """Reads with 1, 2, 63, 64, 65 and 1 500 tuples, in shuffled order; the 1 500 sit on a poly-A target, so that all of
    them tie through targetsub."""
    rng = random.Random(6)
    reads = sorted({rand_seq(rng, 40, b"CGT") for _ in range(5)} | {b"A" * 30})
    targets = [b"A" * 2000, rand_seq(rng, 300, b"ACGT")]
    rests = rests_of(targets, [b"polyA", b"rnd"])
    hits = [(0, 0, p, p % 2) for p in range(1500)]
    for r, n in zip(range(1, 6), (1, 2, 63, 64, 65)):
        hits += [(r, 1, p, (p * 7) % 5) for p in range(n)]
    rng.shuffle(hits)
    tails = [b"%d\tname%d" % (r + 1, r) for r in range(len(reads))]
    return reads, targets, rests, hits, tails


def test_segments_of_a_shuffled_host_list(eng, segments):
    reads, targets, rests, hits, tails = segments
    assert reads[0] == b"A" * 30
    load(eng, reads, targets, rests, tails)
    check(eng, reads, targets, rests, hits, tails)


def test_text_in_chunks(eng, segments):
    reads, targets, rests, hits, tails = segments
    load(eng, reads, targets, rests, tails)
    exp = oracle_text(reads, targets, rests, hits, tails)
    nl, nb = eng.results_order(np.array(hits, dtype=np.uint32))
    assert nl == len(hits) == 1695
    for step in (1, 7, 64, 1001):
        parts = [eng.results_text(l0, step) for l0 in range(0, nl, step)]
        assert all(p.count(b"\n") == min(step, nl - l0) for p, l0 in zip(parts, range(0, nl, step)))
        assert b"".join(parts) == exp, step
    assert eng.results_text(nl, 5) == b"" and eng.results_text(nl + 1000) == b"" and eng.results_text(3, 0) == b""
    assert eng.results_text(nl - 2, 100) == b"".join(exp.splitlines(True)[-2:])


STAGE_KNOBS = ("MUSC_DEBUG_STAGE_BYTES", "MUSC_DEBUG_STAGE_LINES")


@contextlib.contextmanager
def staged(eng, stage_bytes, stage_lines):
    """The text calls of `eng` with a staging buffer of `stage_bytes` and offset windows of `stage_lines` records, so
    that a small range passes through the host path in many pieces; the defaults are back afterwards."""
    old = {k: os.environ.pop(k, None) for k in STAGE_KNOBS}
    os.environ.update(MUSC_DEBUG_STAGE_BYTES=str(stage_bytes), MUSC_DEBUG_STAGE_LINES=str(stage_lines))
    try:
        eng.reload_env()
        yield
    finally:
        for k in STAGE_KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
        eng.reload_env()


def test_staged_host_path_in_many_pieces(eng, segments):
    """A stage of 256 bytes and windows of 7 lines: the 1 695 lines reach the host in hundreds of pieces.  The fixture's
    own lines are under 100 bytes, so two reads (2 and 64 tuples) get a 300-byte tail here: their lines are larger than
    the stage and go one to a piece, through a staging buffer that grows for them."""
    reads, targets, rests, hits, tails = segments
    tails = list(tails)
    for r in (2, 4):
        tails[r] = b"%d\t" % (r + 1) + b"n" * 300
    load(eng, reads, targets, rests, tails)
    exp = oracle_text(reads, targets, rests, hits, tails)
    lines = exp.splitlines(True)
    assert len(lines) == 1695 and max(len(ln) for ln in lines) > 256 > min(len(ln) for ln in lines)
    nl, nb = eng.results_order(np.array(hits, dtype=np.uint32))
    assert (nl, nb) == (len(lines), len(exp))
    with staged(eng, 256, 7):
        assert eng.results_text() == exp
        for l0, cnt in ((0, 1), (3, 11), (nl - 1, 1)):
            assert eng.results_text(l0, cnt) == b"".join(lines[l0:l0 + cnt]), l0
    assert eng.results_text() == exp  # the knobs unset: the defaults are back


def test_device_destinations_at_every_alignment(eng, segments):
    import torch
    reads, targets, rests, hits, tails = segments
    load(eng, reads, targets, rests, tails)
    exp = oracle_text(reads, targets, rests, hits, tails)
    nl, _ = eng.results_order(np.array(hits, dtype=np.uint32))
    nb = ctypes.c_uint64()
    for a in range(4):
        for l0, cnt in ((0, nl), (3, 11), (nl - 1, 1)):
            want = eng.results_text(l0, cnt)  # (compared with the oracle's bytes by test_text_in_chunks)
            assert want in exp and len(want) > 0
            d = torch.full((len(want) + 16,), 0xEE, dtype=torch.uint8, device="cuda")
            rc = eng._lib.musc_results_text(eng._h, l0, cnt, d.data_ptr() + 4 + a, len(want), 1, ctypes.byref(nb))
            assert rc == 0, eng._lib.musc_last_error(eng._h)
            torch.cuda.synchronize()
            h = d.cpu().numpy().tobytes()
            assert nb.value == len(want) and h[4 + a:4 + a + len(want)] == want, (a, l0)
            assert set(h[:4 + a]) == {0xEE} and set(h[4 + a + len(want):]) == {0xEE}, (a, l0)


def test_text_refusals(eng, segments):
    """Capacity one byte short: code 2, nothing written, *nbytes = 0.  dst = NULL: the size of the range."""
    reads, targets, rests, hits, tails = segments
    load(eng, reads, targets, rests, tails)
    exp = oracle_text(reads, targets, rests, hits, tails)
    eng.results_order(np.array(hits, dtype=np.uint32))
    nb = ctypes.c_uint64(77)
    buf = np.full(len(exp) + 8, 0xEE, dtype=np.uint8)
    rc = eng._lib.musc_results_text(eng._h, 0, 1 << 62, buf.ctypes.data, len(exp) - 1, 0, ctypes.byref(nb))
    assert rc == 2 and b"capacity" in eng._lib.musc_last_error(eng._h) and nb.value == 0
    assert set(buf.tolist()) == {0xEE}
    nb.value = 77
    rc = eng._lib.musc_results_text(eng._h, 0, 1 << 62, None, 0, 0, ctypes.byref(nb))
    assert rc == 0 and nb.value == len(exp)
    assert set(buf.tolist()) == {0xEE}
    rc = eng._lib.musc_results_text(eng._h, 0, 1 << 62, buf.ctypes.data, len(exp), 0, ctypes.byref(nb))
    assert rc == 0 and nb.value == len(exp) and buf[:nb.value].tobytes() == exp


def test_offsets_beyond_four_gib(eng):
    """One read with a 4 000-byte tail and 1.1 M hits on a poly-A target: more than 2^32 bytes of text.  Only the lines
    around byte 2^32 and the last 100 are rendered and compared."""
    n = 1100000
    reads = [b"A" * 30]
    targets = [b"A" * (n + 30)]
    rests = rests_of(targets, [b"polyA"])
    tails = [b"1\t" + b"n" * 3998]
    load(eng, reads, targets, rests, tails)
    hits = np.zeros((n, 4), dtype=np.uint32)
    hits[:, 2] = np.random.default_rng(0).permutation(n)
    nl, nb = eng.results_order(hits)
    order = sorted(range(n), key=str)  # every span is 30 A: the position's decimal text decides
    lens = np.array([len(str(p)) for p in order], dtype=np.int64) + (30 + 1 + 30 + 1 + 1 + 1 + 1 + len(rests[0]) + 1 + 4000 + 1)
    ends = np.cumsum(lens)
    assert nl == n and nb == int(ends[-1]) and nb > (1 << 32) + (1 << 20)
    k = int(np.searchsorted(ends, 1 << 32))
    for l0, cnt in ((k - 50, 100), (n - 100, 100)):
        exp = oracle_text(reads, targets, rests, [(0, 0, p, 0) for p in order[l0:l0 + cnt]], tails)
        assert eng.results_text(l0, cnt) == exp
    assert [int(h[2]) for h in eng.results_hits()[k - 3:k + 3]] == order[k - 3:k + 3]


def test_tails(eng):
    rng = random.Random(8)
    reads = sorted(rand_seq(rng, 25, b"ACGT") for _ in range(3))
    targets = [rand_seq(rng, 80, b"ACGT")]
    rests = rests_of(targets, [b">gene one"])
    hits = [(r, 0, p, 0) for r in range(3) for p in (0, 11, 55)]
    tails = [b"", b"12\t" + b";".join(b"read%04d" % i for i in range(111))[:997], b"1\tz"]
    assert len(tails[1]) == 1000
    load(eng, reads, targets, rests)  # no read text: six columns
    exp6 = check(eng, reads, targets, rests, hits, None)
    assert all(ln.count(b"\t") == 5 for ln in exp6.split(b"\n")[:-1])
    eng.set_read_text(tails)
    with pytest.raises(MuscatoError):
        eng.results_text()  # the offsets were those of the six-column lines
    exp = check(eng, reads, targets, rests, hits, tails)
    assert reads[0] + b"\t" in exp and exp.split(b"\n")[0].endswith(b"\t")  # an empty tail still has its tab


KINDS = {"narrow": {"MUSC_CONTEXT": "narrow"}, "wide": {"MUSC_CONTEXT": "wide"}, "classic64": {"MUSC_INDEX": "classic64"},
         "lines": {"MUSC_INDEX": "lines"}}


def plain_case():
    """No X, two windows, 60-base reads: fits the 120-base context buckets (and the wide ones when they are forced)."""
    rng = random.Random(5)
    targets = [rand_seq(rng, 300, b"ACGT") for _ in range(20)]
    reads = sorted({mutate(rng, t[p:p + 60], 0.02, b"ACGT") for t in targets for p in (0, 57, 240)})
    return orc.Config(Windows=[0, 10], WindowWidth=12, PMatch=0.95, MinDinuc=2, MaxReadLength=60, MMTol=1), reads, targets


def test_resident_list_must_be_current_and_device_lists_aligned(eng):
    """results_order(None) takes the list of the last pass: after a read or a target load there is no such list until the
    next match.  A device list is read with 16-byte loads: a pointer that is not so aligned is refused."""
    import torch
    ocfg, reads, targets = plain_case()
    cfg = Config(Windows=ocfg.Windows, WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                 MaxReadLength=ocfg.MaxReadLength, MaxMatches=ocfg.MaxMatches, MMTol=ocfg.MMTol, MatchMode=ocfg.MatchMode)
    rests = rests_of(targets, [b"g%d" % g for g in range(len(targets))])
    load(eng, reads, targets, rests)
    with pytest.raises(MuscatoError, match="resident tuple list"):
        eng.results_order(None)  # nothing has been matched on these reads and targets
    n = eng.match_device(cfg, apply_mmtol=True)
    assert eng.results_order(None)[0] == n > 0
    eng.set_gene_text(rests)  # a new text leaves the list as it was
    assert eng.results_order(None)[0] == n
    eng.load_reads(reads[:-1])
    with pytest.raises(MuscatoError, match="resident tuple list"):
        eng.results_order(None)
    eng.load_reads(reads)
    eng.match_device(cfg, apply_mmtol=True)
    eng.load_targets(targets)
    eng.set_gene_text(rests)
    with pytest.raises(MuscatoError, match="resident tuple list"):
        eng.results_order(None)
    d = torch.zeros(12, dtype=torch.int32, device="cuda")  # (read 0, gene 0, pos 0, nmiss 0) twice, one word in
    nl, nb = ctypes.c_uint64(), ctypes.c_uint64()
    assert eng._lib.musc_results_order(eng._h, d.data_ptr() + 4, 2, 1, ctypes.byref(nl), ctypes.byref(nb)) == 2
    assert b"16-byte aligned" in eng._lib.musc_last_error(eng._h)
    assert eng._lib.musc_results_order(eng._h, d.data_ptr(), 2, 1, ctypes.byref(nl), ctypes.byref(nb)) == 0 and nl.value == 2


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_list_of_a_real_pass(eng, kind):
    """The random cases of tests/cases.py: match, then order the list the pass left on the device."""
    old = {k: os.environ.pop(k, None) for k in ("MUSC_CONTEXT", "MUSC_INDEX")}
    os.environ.update(KINDS[kind])
    seen = set()
    try:
        eng.reload_env()
        for seed in (None, 1, 3, 12):
            ocfg, reads, targets = make_case(seed) if seed is not None else plain_case()
            cfg = Config(Windows=ocfg.Windows, WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                         MaxReadLength=ocfg.MaxReadLength, MaxMatches=ocfg.MaxMatches, MMTol=ocfg.MMTol, MatchMode=ocfg.MatchMode)
            rests = rests_of(targets, [b"gene_%d" % (g % 7) for g in range(len(targets))])
            tails = [b"%d\tr%d" % (1 + i % 3, i) for i in range(len(reads))]
            absent = (len(targets) - 1,)
            load(eng, reads, targets, rests, tails, absent)
            n = eng.match_device(cfg, apply_mmtol=True)
            fed = np.zeros((n, 4), dtype=np.uint32)
            if n:
                eng.hits_to(fed.ctypes.data, n, False)
            seen.add(eng.stats()["index_kind"])
            exp = oracle_text(reads, targets, rests, fed, tails, absent)
            nl, nb = eng.results_order(None)
            assert (nl, nb) == (exp.count(b"\n"), len(exp))
            assert eng.results_text() == exp
    finally:
        for k in ("MUSC_CONTEXT", "MUSC_INDEX"):
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
        eng.reload_env()
    if kind == "classic64":
        assert seen == {0}
    elif kind == "lines":
        assert seen == {3}
    else:
        assert (1 if kind == "narrow" else 2) in seen, seen
