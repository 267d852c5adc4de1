"""The nonmatch FASTQ, genestats and readstats made on the device (musc_side_*) against the reference's
text tools.

The expected bytes never come from the code under test: results.txt is oracle.muscato_oracle.results_text over the fed
tuples (through test_gpu_results.oracle_text, which puts the test's own tails on the lines), the nonmatch text is
oracle.muscato_oracle.nonmatch_text of it, and the two stats texts are expected_genestats / expected_readstats of
tests/test_cli.py.  A read is (sequence, count, names); its tail on the device is ``count\\tnames``.

Two limits of those text tools shape the cases.  nonmatch_text indexes the token without looking, so reads whose
``names`` hold no token (which the device skips, as the CLI does) are left out of the list it is given.  And the stats
tools cut results.txt into lines at every \\n and \\r, so a token that ends at one of those two bytes is given to
unmatched reads only, where just the nonmatch text shows it; the other four whitespace bytes also end tokens of matched
reads."""
import ctypes
import random

import numpy as np
import pytest

from muscato_amd import Config, Engine, MuscatoError
from oracle import muscato_oracle as orc

from cases import make_case, rand_seq
from test_cli import expected_genestats, expected_readstats
from test_gpu_results import load, oracle_text, plain_case, rests_of, staged

pytestmark = pytest.mark.gpu

TEXTS = ("nonmatch", "genestats", "readstats")
WS = [b" ", b"\t", b"\n", b"\x0b", b"\x0c", b"\r"]


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


def tails_of(R):
    return [b"%d\t%s" % (c, n) for _, c, n in R]


def expected(R, targets, rests, hits, absent=()):
    """(nonmatch, genestats, readstats) of the reference's tools over the oracle's results.txt."""
    reads = [r for r, _, _ in R]
    res = oracle_text(reads, targets, rests, hits, tails_of(R), absent)
    ureads = [orc.UniqueRead(r, c, n) for r, c, n in R if n.split()]
    return orc.nonmatch_text(res, ureads), expected_genestats(res), expected_readstats(res)


def text_fn(eng, which):
    return getattr(eng, which + "_text")


def nrecords(which, text):
    return text.count(b"\n") // (4 if which == "nonmatch" else 1)


def check(eng, R, targets, rests, hits, absent=(), steps=()):
    """Load, order `hits`, prepare, and compare the three texts (whole, and in ranges of `steps` records) and the
    counts with the reference's."""
    reads = [r for r, _, _ in R]
    exp = dict(zip(TEXTS, expected(R, targets, rests, hits, absent)))
    load(eng, reads, targets, rests, tails_of(R), absent)
    eng.results_order(np.array(hits, dtype=np.uint32).reshape(-1, 4))
    got = eng.side_prepare()
    for which in TEXTS:
        assert text_fn(eng, which)() == exp[which], which
        n = nrecords(which, exp[which])
        assert got[which] == (n, len(exp[which])), which
        for step in steps:
            parts = [text_fn(eng, which)(r0, step) for r0 in range(0, n, step)]
            assert b"".join(parts) == exp[which], (which, step)
            assert all(nrecords(which, p) == min(step, n - r0) for p, r0 in zip(parts, range(0, n, step))), (which, step)
        assert text_fn(eng, which)(n, 5) == b"" and text_fn(eng, which)(0, 0) == b""
    return exp


def distinct_reads(rng, n, L=20, alphabet=b"ACGT"):
    s = set()
    while len(s) < n:
        s.add(rand_seq(rng, L, alphabet))
    return sorted(s)


@pytest.mark.parametrize("form", ["all_matched", "none_matched", "alternating"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_read_counts(eng, n, form):
    rng = random.Random(n)
    targets = [rand_seq(rng, 40, b"ACGT"), rand_seq(rng, 33, b"ACGT")]
    rests = rests_of(targets, [b"ga", b"gb"])
    R = [(r, 1 + i % 3, b"r%d;s%d" % (i, i)) for i, r in enumerate(distinct_reads(rng, n))]
    matched = {"all_matched": range(n), "none_matched": [], "alternating": range(0, n, 2)}[form]
    hits = [(i, i % 2, i % 7, 0) for i in matched]
    exp = check(eng, R, targets, rests, hits)
    if form == "all_matched":
        assert exp["nonmatch"] == b""
    if form == "none_matched":
        assert exp["genestats"] == b"" and exp["readstats"] == b"" and exp["nonmatch"].count(b"\n") == 4 * n


LENS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 253]


def test_read_lengths_and_x(eng):
    """Every length plain and with an X at its first base, its last base and the bases on either side of a 16-base word
    boundary; every third read is matched, the others are rendered from the 2-bit planes."""
    rng = random.Random(3)
    seqs = set()
    for L in LENS:
        base = rand_seq(rng, L, b"ACGT")
        seqs.add(base)
        for xs in ([0], [L - 1], [15, 16], [31, 32, 47, 48]):
            b = bytearray(rand_seq(rng, L, b"ACGT"))
            for p in xs:
                if p < L:
                    b[p] = ord("X")
            seqs.add(bytes(b))
    reads = sorted(seqs)
    assert any(r.startswith(b"X") for r in reads) and any(r.endswith(b"X") for r in reads)
    targets = [rand_seq(rng, 300, b"ACGT")]
    rests = rests_of(targets, [b"t"])
    R = [(r, i + 1, b"name%d" % i) for i, r in enumerate(reads)]
    hits = [(i, 0, i, 1) for i in range(0, len(reads), 3)]
    exp = check(eng, R, targets, rests, hits, steps=(1, 7))
    assert exp["nonmatch"].count(b"X") >= 20


def test_tails(eng):
    """Counts at the digit edges, tokens ended by each whitespace byte, leading blanks, reads without a token (skipped
    in nonmatch, ignored in readstats without splitting a run), a 1 000-byte token, a byte above 0x7F."""
    rng = random.Random(4)
    names = []
    for c in (1, 9, 10, 99, 100, 1000000):
        names.append((c, b"cnt%d" % c))
    for w in WS:  # unmatched reads: all six bytes
        names.append((2, b"end" + w + b"rest"))
        names.append((2, b"tail" + w))
    for w in (b" ", b"\t", b"\x0b", b"\x0c"):  # matched reads: the four that do not end a line
        names.append((3, b"m" + w + b"rest;more"))
    names.append((3, b"mr\r"))  # (\r\n is one line end for the text tools as well)
    names += [(1, b"  lead"), (1, b"\t \x0blead2 x"), (4, b""), (5, b" \t  "), (1, b"T" * 1000), (1, b"T" * 999 + b"\x80"),
              (1, b"caf\xc3\xa9 x"), (7, b"\xff\xfe")]
    # a run "same" that an unmatched read, a read without a token and a read of blanks interrupt, but do not split
    names += [(1, b"same"), (1, b"other"), (1, b"same z"), (1, b""), (1, b"same\ty"), (2, b"   "), (1, b"same")]
    reads = distinct_reads(rng, len(names), 25)
    R = [(r, c, n) for r, (c, n) in zip(reads, names)]
    targets = [rand_seq(rng, 80, b"ACGT"), rand_seq(rng, 80, b"ACGT")]
    rests = rests_of(targets, [b"g1", b"g2"])
    run0 = len(names) - 7
    unmatched = set(range(6 + 2 * len(WS))) | {run0 + 1}  # the counts, the six ending bytes, and "other" inside the run
    hits = [(i, i % 2, 3, 0) for i in range(len(names)) if i not in unmatched]
    hits += [(run0, 0, 5, 0)]
    exp = check(eng, R, targets, rests, hits, steps=(1, 7, 64))
    assert b"same\tg1;g2;\n" in exp["readstats"] and exp["readstats"].count(b"same\t") == 1
    assert b"cnt1000000#1000000\n" in exp["nonmatch"] and b"end#2\n" in exp["nonmatch"] and b"tail#2\n" in exp["nonmatch"]
    assert b"T" * 1000 + b"\t" in exp["readstats"] and b"\xff\xfe\t" in exp["readstats"]
    # the reads without a token are in no text at all
    for i, (_, n) in enumerate(names):
        if not n.split():
            assert reads[i] not in exp["nonmatch"]


def test_runs(eng):
    rng = random.Random(5)
    tok = [b"a", b"a", b"b", b"b", b"b", b"c", b"x", b"c", b"d", b"d", b"e", b"", b"e", b"f", b"g", b"f"]
    unmatched = {6, 9}  # c x c: x is unmatched -> one run of c; d d: the second d is unmatched
    reads = distinct_reads(rng, len(tok), 30)
    R = [(r, 1, t + b" zz" if t else b"") for r, t in zip(reads, tok)]
    targets = [rand_seq(rng, 60, b"ACGT") for _ in range(4)]
    rests = rests_of(targets, [b"g3", b"g1", b"g2", b"g1"])
    hits = [(i, g, 1, 0) for i in range(len(tok)) if i not in unmatched for g in range(4) if (i + g) % 3]
    exp = check(eng, R, targets, rests, hits, steps=(1, 7))
    lines = exp["readstats"].split(b"\n")[:-1]
    assert [ln.split(b"\t")[0] for ln in lines] == [b"a", b"b", b"c", b"d", b"e", b"f", b"g", b"f"]


def test_gene_names(eng):
    """One name with two lengths, byte-identical texts, names that are prefixes of one another, and a read whose only
    tuples are of an absent gene: in nonmatch, in neither stats text."""
    rng = random.Random(6)
    reads = distinct_reads(rng, 6, 22)
    t = rand_seq(rng, 50, b"ACGT")
    targets = [t, t[:40], t, t, t + b"A", t, t]
    rests = rests_of(targets, [b"g", b"g", b"g10", b"g9", b"g1", b"g1", b"gone"])
    assert rests[0] != rests[1] and rests[5] != rests[4] and rests[2][:3] == b"g10"
    rests[5] = rests[4]  # byte-identical texts
    R = [(r, i + 1, b"r%d" % i) for i, r in enumerate(reads)]
    hits = [(0, g, 0, 0) for g in range(7)] + [(1, 0, 1, 0), (1, 1, 1, 0), (2, 6, 0, 0), (3, 5, 2, 0), (3, 4, 2, 0), (5, 6, 0, 0), (5, 3, 0, 0)]
    exp = check(eng, R, targets, rests, hits, absent=(6,), steps=(1,))
    assert exp["genestats"] == b"g\t4\t\ng1\t4\t\ng10\t1\t\ng9\t2\t\n"
    assert b"gone" not in exp["genestats"] + exp["readstats"]
    assert reads[2] in exp["nonmatch"] and reads[4] in exp["nonmatch"] and reads[5] not in exp["nonmatch"]
    assert exp["readstats"].startswith(b"r0\tg;g1;g10;g9;\n")


@pytest.mark.parametrize("ntup", [10, 100])
def test_gene_count_digits(eng, ntup):
    reads = [b"A" * 30, b"C" * 30]
    targets = [b"A" * 200, b"C" * 60]
    rests = rests_of(targets, [b"polyA", b"polyC"])
    R = [(reads[0], 1, b"ra"), (reads[1], 1, b"rc")]
    hits = [(0, 0, p, 0) for p in range(ntup)] + [(1, 1, p, 0) for p in range(9)]
    exp = check(eng, R, targets, rests, hits)
    assert exp["genestats"] == b"polyA\t%d\t\npolyC\t9\t\n" % ntup


def test_one_read_with_300_gene_names(eng):
    rng = random.Random(7)
    reads = distinct_reads(rng, 3, 24)
    t = rand_seq(rng, 30, b"ACGT")
    targets = [t] * 320
    rests = rests_of(targets, [b"gene%d" % (g % 300) for g in range(320)])
    R = [(reads[0], 1, b"first"), (reads[1], 2, b"big one"), (reads[2], 3, b"last")]
    order = list(range(320))
    rng.shuffle(order)
    hits = [(0, 5, 0, 0)] + [(1, g, g % 5, 0) for g in order] + [(2, 7, 1, 0), (2, 7, 2, 0)]
    exp = check(eng, R, targets, rests, hits, steps=(1, 7))
    big = exp["readstats"].split(b"\n")[1]
    assert big.startswith(b"big\tgene0;gene1;gene10;gene100;") and big.count(b";") == 300


@pytest.fixture(scope="module")
def mixed():
    """257 reads, two in three matched, some on several genes, tokens shared by neighbours."""
    rng = random.Random(8)
    reads = distinct_reads(rng, 257, 37)
    targets = [rand_seq(rng, 90, b"ACGT") for _ in range(12)]
    rests = rests_of(targets, [b"n%d" % (g % 5) for g in range(12)])
    R = [(r, 1 + i % 11, b"tok%d rest" % (i // 3)) for i, r in enumerate(reads)]
    hits = [(i, (i * 7 + k) % 12, k, k % 2) for i in range(257) if i % 3 for k in range(1 + i % 4)]
    return R, targets, rests, hits


def test_ranges(eng, mixed):
    R, targets, rests, hits = mixed
    check(eng, R, targets, rests, hits, steps=(1, 7, 64))


@pytest.mark.parametrize("stage_bytes,stage_lines", [(256, 7), (1, 1)])
def test_staged_host_path_in_many_pieces(eng, mixed, stage_bytes, stage_lines):
    """A stage of 256 bytes with windows of 7 records, and a stage of one byte with windows of one (every piece is then
    one record, each larger than the stage): the three texts, whole and in three ranges, through the host path."""
    R, targets, rests, hits = mixed
    exp = dict(zip(TEXTS, expected(R, targets, rests, hits)))
    load(eng, [r for r, _, _ in R], targets, rests, tails_of(R))
    eng.results_order(np.array(hits, dtype=np.uint32))
    got = eng.side_prepare()
    with staged(eng, stage_bytes, stage_lines):
        for which in TEXTS:
            assert text_fn(eng, which)() == exp[which], which
            per = 4 if which == "nonmatch" else 1
            lines = exp[which].splitlines(True)
            n = got[which][0]
            assert n == len(lines) // per > 3
            for r0, cnt in ((0, 1), (3, 11), (n - 1, 1)):
                assert text_fn(eng, which)(r0, cnt) == b"".join(lines[per * r0:per * (r0 + cnt)]), (which, r0)
    for which in TEXTS:
        assert text_fn(eng, which)() == exp[which], which  # the knobs unset


def test_device_destinations_at_every_alignment(eng, mixed):
    import torch
    R, targets, rests, hits = mixed
    exp = dict(zip(TEXTS, expected(R, targets, rests, hits)))
    load(eng, [r for r, _, _ in R], targets, rests, tails_of(R))
    eng.results_order(np.array(hits, dtype=np.uint32))
    got = eng.side_prepare()
    nb = ctypes.c_uint64()
    for w, which in enumerate(TEXTS):
        nrec, nbytes = got[which]
        assert nbytes == len(exp[which]) > 0
        for a in range(4):
            for r0, cnt in ((0, nrec), (3, 11), (nrec - 1, 1)):
                want = text_fn(eng, which)(r0, cnt)  # (compared with the reference's bytes by test_ranges)
                assert want in exp[which] and len(want) > 0
                d = torch.full((len(want) + 16,), 0xEE, dtype=torch.uint8, device="cuda")
                rc = eng._lib.musc_side_text(eng._h, w, r0, cnt, d.data_ptr() + 4 + a, len(want), 1, ctypes.byref(nb))
                assert rc == 0, eng._lib.musc_last_error(eng._h)
                torch.cuda.synchronize()
                h = d.cpu().numpy().tobytes()
                assert nb.value == len(want) and h[4 + a:4 + a + len(want)] == want, (which, a, r0)
                assert set(h[:4 + a]) == {0xEE} and set(h[4 + a + len(want):]) == {0xEE}, (which, a, r0)


def test_nonmatch_offsets_beyond_four_gib(eng):
    """1.1 M unmatched 2 000-base reads, loaded packed: more than 2^32 bytes of FASTQ.  The totals are arithmetic on the
    record lengths; only the records around byte 2^32 and the last ones are rendered and compared."""
    n, L = 1100000, 2000
    rng = np.random.default_rng(0)
    packed = rng.integers(0, 256, size=n * L // 4 + 64, dtype=np.uint8)
    eng.load_targets([b"ACGT" * 10])
    eng.load_reads_packed32_ptr(packed.ctypes.data, 0, 0, L, n)
    eng.set_gene_text([b"g\t40"])
    counts = (np.arange(n, dtype=np.int64) * 7919) % 100000 + 1
    tails = [b"%d\tq%d z" % (int(c), i) for i, c in enumerate(counts)]
    eng.set_read_text(tails)
    assert eng.results_order(np.zeros((0, 4), dtype=np.uint32)) == (0, 0)
    got = eng.side_prepare()
    lens = np.array([len(t) - 3 for t in tails], dtype=np.int64) + (2 + L + 3 + L + 1)  # q<i> # <count> \n SEQ \n+\n !..! \n
    ends = np.cumsum(lens)
    assert got["nonmatch"] == (n, int(ends[-1])) and int(ends[-1]) > (1 << 32) + (1 << 20)
    assert got["genestats"] == (0, 0) and got["readstats"] == (0, 0)
    k = int(np.searchsorted(ends, 1 << 32))

    def seq(i):  # (L is a multiple of 4: read i is bytes [i L / 4, (i + 1) L / 4) of the stream, base 0 in the low bits)
        b = packed[i * L // 4:(i + 1) * L // 4]
        return bytes(b"ACGT"[(int(v) >> sh) & 3] for v in b for sh in (0, 2, 4, 6))

    for r0, cnt in ((k - 3, 6), (n - 4, 4), (0, 2)):
        res = b""  # (no read is matched: the reference's tool sees an empty results.txt)
        ur = [orc.UniqueRead(seq(i), int(counts[i]), b"q%d z" % i) for i in range(r0, r0 + cnt)]
        assert eng.nonmatch_text(r0, cnt) == orc.nonmatch_text(res, ur), r0


def _cfg(ocfg):
    return Config(Windows=ocfg.Windows, WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc,
                  MaxReadLength=ocfg.MaxReadLength, MaxMatches=ocfg.MaxMatches, MMTol=ocfg.MMTol, MatchMode=ocfg.MatchMode)


@pytest.mark.parametrize("seed", [2, 3])
def test_list_of_a_real_pass(eng, seed):
    ocfg, reads, targets = make_case(seed)
    rests = rests_of(targets, [b"gene_%d" % (g % 7) for g in range(len(targets))])
    R = [(r, 1 + i % 3, b"r%d;x%d" % (i // 2, i)) for i, r in enumerate(reads)]
    absent = (len(targets) - 1,)
    load(eng, reads, targets, rests, tails_of(R), absent)
    n = eng.match_device(_cfg(ocfg), apply_mmtol=True)
    fed = np.zeros((n, 4), dtype=np.uint32)
    eng.hits_to(fed.ctypes.data, n, False)
    exp = dict(zip(TEXTS, expected(R, targets, rests, fed, absent)))
    assert n > 0 and eng.results_order(None)[0] > 0
    got = eng.side_prepare()
    for which in TEXTS:
        assert text_fn(eng, which)() == exp[which], which
        assert got[which] == (nrecords(which, exp[which]), len(exp[which]))
    assert all(len(exp[w]) > 0 for w in TEXTS)
    p, t = eng.side_ms()
    assert p > 0 and t > 0


def test_refusals(eng):
    ocfg, reads, targets = plain_case()
    cfg = _cfg(ocfg)
    rests = rests_of(targets, [b"g%d" % g for g in range(len(targets))])
    R = [(r, 1, b"r%d" % i) for i, r in enumerate(reads)]
    tails = tails_of(R)
    hits = np.array([(i, i % len(targets), 0, 0) for i in range(0, len(reads), 2)], dtype=np.uint32)
    exp = dict(zip(TEXTS, expected(R, targets, rests, hits)))

    def good():
        """A correct sequence still works, and returns these inputs' texts, not anything older."""
        eng.results_order(hits)
        eng.side_prepare()
        for which in TEXTS:
            assert text_fn(eng, which)() == exp[which], which

    def refused(match, code=2):
        with pytest.raises(MuscatoError, match=match) as ei:
            eng.side_prepare()
        assert "(%d)" % code in str(ei.value)
        for which in TEXTS:
            with pytest.raises(MuscatoError, match="nothing prepared"):
                text_fn(eng, which)()

    with Engine(0) as fresh:  # before anything at all
        with pytest.raises(MuscatoError, match="no ordered list"):
            fresh.side_prepare()
        with pytest.raises(MuscatoError, match="nothing prepared"):
            fresh.nonmatch_text()
    load(eng, reads, targets, rests)  # no read text
    refused("no ordered list")
    eng.results_order(hits)
    refused("no read text")
    eng.set_read_text(tails)
    refused("no ordered list")  # a new text invalidates the order
    good()
    eng.load_reads(reads[:-1])
    refused("no ordered list")
    eng.load_reads(reads)
    eng.set_read_text(tails)
    good()
    eng.load_targets(targets)
    refused("no ordered list")
    eng.set_gene_text(rests)
    refused("no ordered list")
    good()
    eng.set_gene_text(rests)
    refused("no ordered list")
    good()
    assert eng.match_device(cfg, apply_mmtol=True) > 0
    refused("a pass ran after")
    good()
    # a gene text outside the simple form: its own code, and the context is as good as before
    for bad in (b"g 0\t300", b"g0\t3\t00", b"\t300", b"g0\t", b"g0", b"g\x0b0\t300"):
        eng.set_gene_text([bad] + rests[1:])
        eng.results_order(hits)
        assert len(eng.results_text()) > 0
        refused("not in the simple form", code=12)
        assert len(eng.results_text()) > 0  # results.txt does not need the form
    eng.set_gene_text([b"g 0\t300"] + rests[1:], [True] + [False] * (len(rests) - 1))  # an absent gene's text is not looked at
    eng.results_order(hits)
    eng.side_prepare()
    eng.set_gene_text(rests)
    good()
    # capacity one byte short: an error that writes nothing; which = 3
    nb = ctypes.c_uint64()
    for w, which in enumerate(TEXTS):
        buf = np.full(len(exp[which]) + 8, 0xEE, dtype=np.uint8)
        rc = eng._lib.musc_side_text(eng._h, w, 0, 1 << 62, buf.ctypes.data, len(exp[which]) - 1, 0, ctypes.byref(nb))
        assert rc == 2 and b"capacity" in eng._lib.musc_last_error(eng._h) and nb.value == 0
        assert set(buf.tolist()) == {0xEE}
        rc = eng._lib.musc_side_text(eng._h, w, 0, 1 << 62, buf.ctypes.data, len(exp[which]), 0, ctypes.byref(nb))
        assert rc == 0 and nb.value == len(exp[which]) and buf[:nb.value].tobytes() == exp[which]
    for w in (3, -1):
        assert eng._lib.musc_side_text(eng._h, w, 0, 1, None, 0, 0, ctypes.byref(nb)) == 2
        assert b"no such text" in eng._lib.musc_last_error(eng._h)
    good()
