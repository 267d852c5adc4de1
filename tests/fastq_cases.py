"""Seeded FASTQ texts and a pure-Python model of the record table the device stage builds from them.

The model follows bufio.ScanLines (utils/fastq.go:35-61): a line ends at '\\n', one trailing '\\r' is dropped, a last line
without '\\n' is a line, records are four lines and an incomplete last record is dropped -- oracle.read_fastq does the
same but for the '\\r' -- and cmd/muscato_prep_reads/main.go:46-92: MinReadLength on the raw length, every byte that is
none of A C G T becomes X, the rest is cut at MaxReadLength.  tests/test_fastq_cases.py holds it to the oracle and
asserts what each case covers; tests/test_gpu_fastq.py holds musc_reads_prep_fastq to it."""
import random
from dataclasses import dataclass, field
from typing import List

import numpy as np

# bytes a lane, a wave and a workgroup of the newline pass own (kernels_fastq.hpp: FQ_LANE_BYTES, x 64, FQ_TILE_BYTES)
STRIDES = (16, 1024, 4096)
LANE, WAVE, TILE = STRIDES

SUBX = bytes(c if c in b"ACGT" else ord("X") for c in range(256))


def scan_lines(raw: bytes):
    """[(begin, end)] of every line, end after the '\\r' rule."""
    spans, pos, n = [], 0, len(raw)
    while pos < n:
        e = raw.find(b"\n", pos)
        end = n if e < 0 else e
        stop = end - 1 if end > pos and raw[end - 1] == 13 else end
        spans.append((pos, stop))
        if e < 0:
            break
        pos = e + 1
    return spans


@dataclass
class Model:
    n_records: int = 0
    n_short: int = 0
    max_len: int = 0
    name_off: List[int] = field(default_factory=list)  # the kept reads, in file order
    name_len: List[int] = field(default_factory=list)
    seq_off: List[int] = field(default_factory=list)
    seq_len: List[int] = field(default_factory=list)    # the prepared length
    seqs: List[bytes] = field(default_factory=list)     # the prepared sequences
    names: List[bytes] = field(default_factory=list)    # after the \r rule, before the 1000-byte rule

    @property
    def n_reads(self):
        return len(self.seqs)


def model(raw: bytes, min_len: int, max_len: int) -> Model:
    m = Model()
    lines = scan_lines(raw)
    m.n_records = len(lines) // 4
    for r in range(m.n_records):
        (nb, ne), (sb, se) = lines[4 * r], lines[4 * r + 1]
        if se - sb < min_len:
            m.n_short += 1
            continue
        ln = min(se - sb, max_len)
        m.name_off.append(nb)
        m.name_len.append(ne - nb)
        m.seq_off.append(sb)
        m.seq_len.append(ln)
        m.seqs.append(raw[sb:sb + ln].translate(SUBX))
        m.names.append(raw[nb:ne])
        m.max_len = max(m.max_len, ln)
    return m


def short_name(name: bytes) -> bytes:
    """cmd/muscato_prep_reads/main.go:76-79"""
    return name[:995] + b"..." if len(name) > 1000 else name


def join_names(names) -> bytes:
    """The names of one group as reads_sorted.txt.sz holds them: the `seq\\tname` lines of a sequence sort by name, a name
    ends at its first tab, 1000 bytes in all (cmd/muscato_uniqify/main.go:83-135)."""
    na = b";".join(n.split(b"\t")[0] for n in sorted(short_name(n) for n in names))
    return na[:996] + b"..." if len(na) > 1000 else na


def unique(m: Model):
    """[(seq, count, names)] in bytewise order of the sequences."""
    groups = {}
    for s, n in zip(m.seqs, m.names):
        groups.setdefault(s, []).append(n)
    return [(s, len(groups[s]), join_names(groups[s])) for s in sorted(groups)]


@dataclass
class Case:
    name: str
    raw: bytes
    min_len: int
    max_len: int
    mark: tuple = ()  # what tests/test_fastq_cases.py asserts about the text


def bases(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def record(name, seq, plus=b"+", qual=None, eol=b"\n"):
    return b"@" + name + eol + seq + eol + plus + eol + (b"I" * len(seq) if qual is None else qual) + eol


def some_records(rng, n, tag, lo=20, hi=80):
    return b"".join(record(b"%s%d" % (tag, i), bases(rng, rng.randint(lo, hi))) for i in range(n))


def boundary_case(stride, delta, kind):
    """The newline that ends a line of kind `kind` (0 name, 1 sequence, 2 plus, 3 quality) sits at byte stride - 1 + delta:
    the last byte of a lane's, a wave's or a workgroup's span, or the first of the next."""
    rng = random.Random(1000 * stride + 10 * delta + kind)
    at = stride - 1 + delta
    head = some_records(rng, max(0, (at - 700) // 120), b"h") if at > 1500 else b""
    assert len(head) <= at - 600 or not head
    parts = [b"@", b"A", b"+", b"I"]  # the shortest lines in front of the padded one
    pad = at - len(head) - sum(len(p) + 1 for p in parts[:kind])
    assert pad >= 1
    parts[kind] = {0: b"@" + b"n" * (pad - 1), 1: bases(rng, pad), 2: b"+" + b"p" * (pad - 1), 3: b"I" * pad}[kind]
    raw = head + b"".join(p + b"\n" for p in parts) + some_records(rng, 3, b"t")
    assert raw[at] == 10 and raw[:at].count(b"\n") % 4 == kind
    return Case("nl_%d%+d_k%d" % (stride, delta - 1, kind), raw, 1, 100, ("newline", at, kind))


def sized_case(n):
    """Exactly n bytes: records cut off wherever byte n falls."""
    rng = random.Random(n)
    raw = b""
    while len(raw) < n:
        raw += some_records(rng, 8, b"s")
    return Case("size_%d" % n, raw[:n], 1, 60, ("size", n))


SIZES = (0, 1, 15, 16, 17, TILE - 1, TILE + 1, 2 * TILE - 1, 2 * TILE + 1, 3 * TILE - 1, 3 * TILE + 1)


def big_text():
    """About 9 MB: more tiles than one block of the scan takes (2048), so the scan of the tile counts has two levels.
    40 000 reads of 100 bases drawn from 6 000 sequences."""
    rs = np.random.RandomState(5)
    pool = np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, size=(6000, 100))]
    pick = rs.randint(0, 6000, size=40000)
    qual = b"F" * 100
    return b"".join(b"@big_read_%07d/1 lane:3 tile:%05d\n%s\n+\n%s\n" % (i, pick[i], pool[pick[i]].tobytes(), qual)
                    for i in range(40000))


_CASES = None


def cases() -> List[Case]:
    global _CASES
    if _CASES is not None:
        return _CASES
    rng = random.Random(77)
    out = [boundary_case(s, d, k) for s in STRIDES for d in (0, 1) for k in range(4)]
    out += [sized_case(n) for n in SIZES]
    # sixteen newlines that fill one lane's chunk: empty names and empty sequences among them
    first = record(b"r0", b"ACGTACGTAC", qual=b"IIIIIIIIII")
    first = first[:-1] + b"I" * (2 * LANE - len(first)) + b"\n"  # 32 bytes
    out.append(Case("nl_run16", first + b"\n" * LANE + some_records(rng, 3, b"a"), 0, 100, ("run", 2 * LANE)))
    body = some_records(rng, 5, b"d")
    out.append(Case("no_trailing_newline", body[:-1], 1, 100, ("lines", 20, False)))
    for k in (1, 2, 3):
        dang = b"".join([b"@dangling\n", b"ACGTACGTACGTACGTACGTACGT\n", b"+\n"][:k])
        out.append(Case("dangling_%d" % k, body + dang, 1, 100, ("lines", 20 + k, True)))
        out.append(Case("dangling_%d_open" % k, body + dang[:-1], 1, 100, ("lines", 20 + k, False)))
    out.append(Case("empty_lines", record(b"", b"ACGT")[1:] + record(b"e1", b"") + b"\n\n\n\n" + record(b"e3", b"GGCC"), 0, 100,
                    ("empty",)))
    out.append(Case("crlf", b"".join(record(b"c%d" % i, bases(rng, 30 + i), eol=b"\r\n") for i in range(6)), 1, 100, ("crlf",)))
    out.append(Case("lone_cr", record(b"cr\rin name", b"ACGT\rACGTACGT") + record(b"two\r", b"ACGTACGTAC\r\r", eol=b"\r\n") +
                    record(b"cr_only", b"\r"), 1, 100, ("lone_cr",)))
    out.append(Case("at_lines", record(b"a0", b"ACGTACGTACGT", plus=b"@a0 again", qual=b"@IIIIIIIIIII") +
                    record(b"a1", b"TTTTACGTACGT", plus=b"+", qual=b"@@@@@@@@@@@@"), 1, 100, ("at",)))
    out.append(Case("min_max", b"".join(record(b"m%d" % n, bases(rng, n)) for n in (19, 20, 50, 51, 35)), 20, 50,
                    ("lengths", (19, 20, 50, 51))))
    out.append(Case("long_read", some_records(rng, 2, b"l") + record(b"long", bases(rng, 10000), qual=b"I") + some_records(rng, 2, b"m"),
                    1, 65535, ("long", 10000)))
    out.append(Case("odd_bytes", record(b"o0", b"acgtACGTnNacgt") + record(b"o1", b"AC\x00GT\xffAC\x80GT") +
                    record(b"o2", b"ACGTXXACGT..ACGT") + record(b"o3", bytes(range(32, 127)).replace(b"\n", b"")), 1, 200, ("odd",)))
    seq = bases(rng, 40)
    out.append(Case("names", record(b"n" * 999, seq) + record(b"m" * 1000, seq) + record(b"tab\there\tand here", seq) +
                    record(b"\tleading tab", bases(rng, 40)) + b"".join(record(b"q%02d" % i + b"x" * 120, seq) for i in range(9)),
                    1, 100, ("names",)))
    dup = bases(rng, 33)
    out.append(Case("dup_names", record(b"zeta", dup) + record(b"b\tzz", dup) + record(b"alpha", bases(rng, 33)) +
                    record(b"a\tyy", dup) + record(b"b", dup) + record(b"Zed", dup) + record(b"b!", dup), 1, 100, ("dups",)))
    out.append(Case("big", big_text(), 1, 100, ("big",)))
    _CASES = out
    return out


def small_cases():
    return [c for c in cases() if c.name != "big"]
