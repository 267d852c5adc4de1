"""Inputs of the target-preparation tests (tests/test_targets_prep_cases.py without a GPU, tests/test_gpu_targets_prep.py
and tests/test_cli_prep_targets.py with one): a seeded case generator and a pure-Python model of the stage.

The model states cmd/muscato_prep_targets/main.go:48-213 in the parallel form DESIGN.md 22 gives -- lines under
bufio.ScanLines' rule, the text format's records as the lines below the first stop line, FASTA records as the spans
between header lines -- and shares nothing with oracle/muscato_oracle.py, to which tests/test_targets_prep_cases.py
holds it.  Every case carries the tags of the list REQUIRED that it covers; the same test asserts that no tag is left.

Boundary tags: `<byte>@<B>:<where>` with byte in nl, tab, gt; B in 16 (a lane), 1024 (a wave), 4096 (a tile); where =
last (the byte at B - 1), first (at B), straddle (at B - 1 and at B)."""
import functools
import random
from collections import namedtuple

Case = namedtuple("Case", "name text fasta covers")
Model = namedtuple("Model", "seqs ids n_lines stop_line n_dropped n_subx refused")  # refused: the first empty FASTA line, or None

NO_STOP = 2 ** 64 - 1
_SUBX = bytes(c if c in b"ACGT" else ord("X") for c in range(256))
_COMP = bytes({65: 84, 84: 65, 67: 71, 71: 67, 88: 88}.get(c, 0) for c in range(256))

BOUNDARIES = (16, 1024, 4096)
LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 9, 10, 99, 100, 999, 1000, 99999, 100000)
COUNTS = (0, 1, 9, 10, 11, 99, 100, 101, 255, 256, 257, 2100)  # 2100: the scans of the record tables take two levels

REQUIRED = tuple(
    ["%s@%d:%s" % (b, B, w) for b in ("nl", "tab", "gt") for B in BOUNDARIES for w in ("last", "first", "straddle")] +
    ["nl8_lane", "rec3_lane", "line_3x4096p5", "rec_300_lines", "rec_3_tiles", "hdr_5000", "gt_alone",
     "crlf", "cr_inside", "no_final_nl", "lone_cr_last:fasta", "lone_cr_last:text",
     "headless", "nobases_start", "nobases_mid", "nobases_end", "two_headers", "last_raw", "earlier_raw",
     "empty_first", "empty_mid", "empty_last", "gt_inside",
     "no_tab", "two_tabs", "empty_name", "empty_seq", "stop_line0", "stops_3_tiles", "no_stop", "empty"] +
    ["len:%d:%s" % (n, f) for n in LENGTHS for f in ("fasta", "text") if not (n == 0 and f == "fasta")] +
    ["nrec:%d:%s" % (n, f) for n in COUNTS for f in ("fasta", "text")])


# ---------------------------------------------------------------- the model

def lines_of(text):
    """bufio.ScanLines: a line ends at \\n, one trailing \\r is dropped, an unterminated last line is a line, nothing
    follows a final \\n."""
    out, pos, n = [], 0, len(text)
    while pos < n:
        e = text.find(b"\n", pos)
        end = n if e < 0 else e
        out.append(text[pos:end - 1] if end > pos and text[end - 1:end] == b"\r" else text[pos:end])
        if e < 0:
            break
        pos = e + 1
    return out


def oracle_text(text):
    """What the tests hand the oracle, which has no \\r rule: the text after bufio's rule."""
    return b"".join(line + b"\n" for line in lines_of(text))


def _emit(records, rev):
    """records: (name, forward sequence).  -> the sequence lines and the id lines, numbers counting both strands."""
    seqs, ids = [], []
    for name, s in records:
        for strand in range(2 if rev else 1):
            seqs.append(s[::-1].translate(_COMP) if strand else s)
            ids.append(b"%011d\t%s%s\t%d" % (len(ids), name, b"_r" if strand else b"", len(s)))
    return seqs, ids


def model(text, fasta, rev):
    lines = lines_of(text)
    n = len(lines)
    if not fasta:
        stop = min((k for k, l in enumerate(lines) if len(l) == 0 or l.count(b"\t") != 1), default=NO_STOP)
        recs, nsub = [], 0
        for l in lines[:min(stop, n)]:
            t = l.index(b"\t")
            raw = l[t + 1:]
            s = raw.translate(_SUBX)
            nsub += sum(a != b for a, b in zip(raw, s))
            recs.append((l[:t], s))
        seqs, ids = _emit(recs, rev)
        return Model(seqs, ids, n, stop, 0, nsub, None)
    empty = min((k for k, l in enumerate(lines) if len(l) == 0), default=None)
    if empty is not None:
        return Model([], [], n, NO_STOP, 0, 0, empty)
    headers = [k for k, l in enumerate(lines) if l[:1] == b">"]
    # group 0: the lines in front of the first header, with the empty name; group g: header g and the lines up to the next
    bounds = [0] + headers + [n]
    recs, nsub, dropped = [], 0, 0
    for g in range(len(bounds) - 1):
        raw = b"".join(lines[bounds[g] + (1 if g else 0):bounds[g + 1]])
        if not raw:
            dropped += 1 if g else 0
            continue
        if g == len(bounds) - 2:  # it reaches the end of the input with bases: not substituted
            s = raw
        else:
            s = raw.translate(_SUBX)
            nsub += sum(a != b for a, b in zip(raw, s))
        recs.append((lines[bounds[g]] if g else b"", s))
    seqs, ids = _emit(recs, rev)
    return Model(seqs, ids, n, NO_STOP, dropped, nsub, None)


def texts_of(m):
    """The two prepared texts of a model: every line with its newline."""
    return b"".join(s + b"\n" for s in m.seqs), b"".join(s + b"\n" for s in m.ids)


# ---------------------------------------------------------------- the cases

def _bases(rng, n, odd=0.0):
    return bytes(rng.choice(b"NnX-") if odd and rng.random() < odd else rng.choice(b"ACGT") for _ in range(n))


def _boundary_cases(rng):
    out = []
    for B in BOUNDARIES:
        for where in ("last", "first", "straddle"):
            P = B - 1 if where != "first" else B  # the first of the one or two bytes
            two = where == "straddle"
            tag = lambda b: {"%s@%d:%s" % (b, B, where)}
            name = "%d_%s" % (B, where)
            # FASTA.  newline: a data line that ends at P (straddle: an empty line follows -- the call is refused)
            out.append(Case("fa_nl_" + name, b">h\n" + _bases(rng, P - 3) + b"\n" + (b"\n" if two else b"") + b"CGT\n>t\nAC\n", True, tag("nl")))
            # tab: data in a sequence line (X), and in the last record as it is
            out.append(Case("fa_tab_" + name, b">h\n" + _bases(rng, P - 3) + (b"\t\t" if two else b"\t") + b"CG\n>t\tu\nA\tC\n", True, tag("tab")))
            # '>': a header that begins at P (straddle: the header ">>x")
            out.append(Case("fa_gt_" + name, b">a\n" + _bases(rng, P - 4) + b"\n" + (b">>x" if two else b">x") + b"\nGATTACA\n", True, tag("gt")))
            # text format.  newline: a record that ends at P (straddle: an empty line, the stop line)
            out.append(Case("tx_nl_" + name, b"n\t" + _bases(rng, P - 2) + b"\n" + (b"\n" if two else b"") + b"m\tCGN\n", False, tag("nl")))
            # tab: the name has P bytes (straddle: two tabs, so line 0 is the stop line)
            out.append(Case("tx_tab_" + name, b"q" * P + (b"\t\t" if two else b"\t") + b"ACGT\nz\tCC\n", False, tag("tab")))
            # '>': data of the sequence
            out.append(Case("tx_gt_" + name, b"n\t" + _bases(rng, P - 2) + (b">>" if two else b">") + b"C\nm\tG\n", False, tag("gt")))
    return out


def _fasta(records, width=60, crlf=False):
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for name, s in records:
        out.append(name + nl)
        out += [s[i:i + width] + nl for i in range(0, len(s), width)]
    return b"".join(out)


def _text(records, crlf=False):
    nl = b"\r\n" if crlf else b"\n"
    return b"".join(name + b"\t" + s + nl for name, s in records)


def _named(rng, lens, odd=0.1):
    return [(b">g%d some text" % i, _bases(rng, L, odd)) for i, L in enumerate(lens)]


@functools.lru_cache(maxsize=None)
def all_cases():
    rng = random.Random(20260222)
    C = _boundary_cases(rng)
    add = lambda name, text, fasta, *tags: C.append(Case(name, bytes(text), fasta, set(tags)))

    # many newlines per lane (the lane is bytes [16, 32) of the text)
    add("fa_nl8", b">h\n" + b"A" * 12 + b"\n" + b"A\n" * 8 + b">t\nAC\n", True, "nl8_lane")
    add("tx_nl8", b"n\t" + b"A" * 13 + b"\n" + b"\t\n" * 8 + b"t\tAC\n", False, "nl8_lane", "empty_name", "empty_seq")
    add("fa_rec3", b">h\n" + b"A" * 12 + b"\n" + b">a\nA\n" * 3 + b"C\n", True, "rec3_lane")

    # long and fragmented records
    long_line = _bases(rng, 3 * 4096 + 5, 0.05)
    add("fa_long_line", b">one line\n" + long_line + b"\n>tail\nACGT\n", True, "line_3x4096p5")
    add("fa_long_line_last", b">one line\n" + long_line, True, "line_3x4096p5", "no_final_nl")
    add("tx_long_line", b"a\tAC\none line\t" + long_line + b"\nz\tGG\n", False, "line_3x4096p5")
    frag = [_bases(rng, rng.randint(1, 3), 0.1) for _ in range(300)]
    add("fa_300_lines", b">a\nAC\n>fragmented\n" + b"\n".join(frag) + b"\n>z\nGT\n", True, "rec_300_lines")
    add("fa_3_tiles", _fasta([(b">a", _bases(rng, 100)), (b">three tiles", _bases(rng, 9000, 0.02)), (b">z", _bases(rng, 70, 0.3))]), True, "rec_3_tiles")
    hdr = b">" + bytes(rng.choice(b"ab \t\tXYZ_|") for _ in range(4999))
    add("fa_hdr_5000", b">a\nACGT\n" + hdr + b"\nACGTNACGT\n>z\nGT\n", True, "hdr_5000")
    add("fa_gt_alone", b">\nACGT\n>\nnnA\n", True, "gt_alone")

    # line endings
    recs = _named(rng, (70, 1, 130, 60))
    add("fa_crlf", _fasta(recs, crlf=True), True, "crlf")
    add("tx_crlf", _text([(n[1:], s) for n, s in recs], crlf=True), False, "crlf")
    add("fa_cr_inside", b">a\rb\nAC\rGT\nA\r\r\n>z\r\r\nG\rT\n", True, "cr_inside")
    add("tx_cr_inside", b"a\rb\tAC\rGT\r\r\nz\r\tG\n", False, "cr_inside")
    add("tx_no_final_nl", b"a\tACGT\nb\tCCNC", False, "no_final_nl", "no_stop")
    add("fa_lone_cr", b">a\nACGT\n\r", True, "lone_cr_last:fasta", "empty_last")
    add("tx_lone_cr", b"a\tACGT\n\r", False, "lone_cr_last:text")

    # FASTA
    add("fa_headless", b"ACnG\nTT\n>a\nACGT\n", True, "headless")
    add("fa_headless_only", b"ACnG\nTT\n", True, "headless", "nrec:1:fasta")
    add("fa_nobases", b">none0\n>a\nACGT\n>none1\n>none2\n>b\nGG\n>none3\n", True, "nobases_start", "nobases_mid", "nobases_end", "two_headers")
    raw = b"acgtNACGT\x00\xffX-ACGT>A"
    add("fa_last_raw", b">first\n" + raw + b"\n>mid\nACGT\n>last\n" + raw + b"\nAC" + raw + b"\n", True, "last_raw", "earlier_raw")
    add("fa_empty_first", b"\n>a\nACGT\n", True, "empty_first")
    add("fa_empty_mid", b">a\nACGT\n>b\n\nAC\n\n", True, "empty_mid")
    add("fa_empty_last", b">a\nACGT\n>b\nAC\n\n", True, "empty_last")
    add("fa_gt_inside", b">a\nAC>GT\nA>\n>b\nG>T\n", True, "gt_inside")

    # text format
    add("tx_no_tab", b"a\tACGT\nno tab here\nb\tGG\n", False, "no_tab")
    add("tx_two_tabs", b"a\tACGT\nb\tGG\tTT\nc\tGG\n", False, "two_tabs")
    add("tx_empty_fields", b"\tACGT\nb\t\n\t\nc\tGG\n", False, "empty_name", "empty_seq", "len:0:text")
    add("tx_stop0", b"no tab\na\tACGT\n", False, "stop_line0", "nrec:0:text")
    many = [(b"g%d" % i, _bases(rng, 50, 0.05)) for i in range(260)]
    stops = _text(many[:100]) + b"first stop\n" + _text(many[100:180]) + b"\n" + _text(many[180:]) + b"x\ty\tz\n" + _text(many[:3])
    add("tx_stops_3_tiles", stops, False, "stops_3_tiles")
    add("empty_fa", b"", True, "empty")
    add("empty_tx", b"", False, "empty")

    # lengths: the small ones together, the decimal widths beside them
    small = [n for n in LENGTHS if n <= 1000]
    add("fa_lens", _fasta(_named(rng, [n for n in small if n]), width=37), True, *["len:%d:fasta" % n for n in small if n])
    add("tx_lens", _text([(b"t%d" % i, _bases(rng, n, 0.1)) for i, n in enumerate(small)]), False, *["len:%d:text" % n for n in small])
    big = [n for n in LENGTHS if n > 1000]
    add("fa_lens_big", _fasta(_named(rng, big, 0.01), width=70), True, *["len:%d:fasta" % n for n in big])
    add("tx_lens_big", _text([(b"t%d" % i, _bases(rng, n, 0.01)) for i, n in enumerate(big)]), False, *["len:%d:text" % n for n in big])

    # record counts
    for n in COUNTS:
        lens = [rng.randint(1, 9) for _ in range(n)]
        add("fa_nrec_%d" % n, _fasta(_named(rng, lens), width=5) if n else b">only\n>headers\n", True, "nrec:%d:fasta" % n)
        if n:
            add("tx_nrec_%d" % n, _text([(b"t%d" % i, _bases(rng, L, 0.1)) for i, L in enumerate(lens)]), False, "nrec:%d:text" % n, "no_stop")

    # small random texts over the bytes that matter
    alphabet = b"ACGTNaX\t\n>\r \x00\xff"
    for i in range(24):
        t = bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 40)))
        add("rand_%d" % i, t, bool(i & 1))
    names = [c.name for c in C]
    assert len(set(names)) == len(names)
    return tuple(C)


def random_texts(seed, count, maxlen=40):
    """The texts of the formulation's check: 0 to maxlen bytes over ACGTNaX, tab, newline, '>', \\r, space, 0x00, 0xFF."""
    rng = random.Random(seed)
    alphabet = b"ACGTNaX\t\n>\r \x00\xff"
    return [bytes(rng.choice(alphabet) for _ in range(rng.randint(0, maxlen))) for _ in range(count)]


def acgtx_only(m):
    return all(set(s) <= set(b"ACGTX") for s in m.seqs)
