"""SAM output as the tests see it, without a GPU and without the library: a pure-Python model of the
format over (reads, targets, id_rests, tails, ordered hits, rev_pairs), an inverse written independently of it (header
and one record back to the read, the target span and the position of a results.txt line), the order of results.txt,
and the seeded cases that tests/test_sam_cases.py, tests/test_gpu_sam.py and tests/test_cli_sam.py share.

A case is a `Case`: reads are distinct and bytewise sorted (as the loaded reads are), targets are over ACGTX, rests[g]
is gene g's ``name\\tlen`` text, absent the genes without an id line, tails[r] read r's ``count\\tnames`` (None: no read
text at all), hits (read, gene, pos, nmiss) in any order."""
import random
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

from oracle import muscato_oracle as orc

WS = b" \t\n\x0b\x0c\r"
HD = b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n"
PG = b"@PG\tID:muscato_amd\tPN:muscato_amd\n"
KEEP_ALL = 1 << 30


class SamRefused(Exception):
    """What musc_sam_prepare answers with code 12."""


@dataclass
class Case:
    name: str
    reads: List[bytes]
    targets: List[bytes]
    rests: List[bytes]
    hits: List[Tuple[int, int, int, int]]
    tails: Optional[List[bytes]] = None
    absent: Tuple[int, ...] = ()
    rev_pairs: bool = False
    refused: bool = False
    note: dict = field(default_factory=dict)


# ---------------------------------------------------------------------------------------------------------------- model
def qname_of(tail):
    if tail is None:
        return b"*"
    i = tail.find(b"\t")
    rest = tail[i + 1:] if i >= 0 else b""
    if rest[:1] in (b"@", b">"):
        rest = rest[1:]
    n = 0
    while n < len(rest) and n < 254 and rest[n:n + 1] != b";" and rest[n] not in WS:
        n += 1
    return rest[:n] or b"*"


def count_of(tail):
    """The value of XC, or None when the record has no XC tag."""
    if tail is None:
        return None
    head = tail.split(b"\t", 1)[0]
    return head if head and all(48 <= c <= 57 for c in head) else None


def rname_of(rest):
    toks = rest.split()
    tok = toks[0] if toks else b""
    return tok[1:] if tok[:1] == b">" else tok


_COMP = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}


def _n(seq):
    return bytes(c if c in b"ACGT" else ord("N") for c in seq)


def _rc_n(seq):
    return bytes(_COMP.get(c, ord("N")) for c in reversed(seq))


def check_refusals(targets, rests, absent, rev_pairs):
    present = [g not in absent for g in range(len(targets))]
    if rev_pairs:
        if len(targets) % 2:
            raise SamRefused("odd number of targets")
        for g in range(0, len(targets), 2):
            if len(targets[g]) != len(targets[g + 1]):
                raise SamRefused("pair of unequal lengths")
    for g in range(len(targets)):
        if not present[g]:
            continue
        if rev_pairs and g % 2:
            if not present[g - 1] or not rname_of(rests[g - 1]):
                raise SamRefused("even partner without a name")
        elif not rname_of(rests[g]):
            raise SamRefused("empty first token")


def header(targets, rests, absent, rev_pairs):
    check_refusals(targets, rests, absent, rev_pairs)
    out = [HD]
    for t in range(len(targets)):
        if t in absent or (rev_pairs and t % 2):
            continue
        out.append(b"@SQ\tSN:%s\tLN:%d\n" % (rname_of(rests[t]), len(targets[t])))
    return b"".join(out + [PG])


def md_of(read, span, rev):
    """(NM, MD) of a span against the first len(span) bases of the read, walked in forward-strand order."""
    steps = range(len(span) - 1, -1, -1) if rev else range(len(span))
    run, d, out = 0, 0, b""
    for j in steps:
        if read[j] == span[j]:
            run += 1
            continue
        d += 1
        base = span[j:j + 1]
        out += b"%d" % run + (_rc_n(base) if rev else _n(base))
        run = 0
    return d, out + b"%d" % run


def records(reads, targets, rests, tails, ordered, rev_pairs, absent=()):
    """One record (bytes, newline included) per tuple of `ordered`, the line order of results.txt."""
    check_refusals(targets, rests, absent, rev_pairs)
    nh = {}
    for h in ordered:
        nh[h[0]] = nh.get(h[0], 0) + 1
    seen, out = {}, []
    for r, g, pos, nmiss in ordered:
        read, L, tl = reads[r], len(reads[r]), len(targets[g])
        S = min(L, tl - pos)
        rev = bool(rev_pairs and g % 2)
        f = g - 1 if rev else g
        hi = seen[r] = seen.get(r, 0) + 1
        tail = tails[r] if tails is not None else None
        if S == 0:
            cigar = b"*"
        else:
            clip = b"%dS" % (L - S) if L > S else b""
            cigar = clip + b"%dM" % S if rev else b"%dM" % S + clip
        d, md = md_of(read, targets[g][pos:pos + S], rev)
        seq = (_rc_n(read) if rev else _n(read)) or b"*"
        cols = [qname_of(tail), b"%d" % ((16 if rev else 0) | (0 if hi == 1 else 256)), rname_of(rests[f]),
                b"%d" % (tl - pos - S + 1 if rev else pos + 1), b"255", cigar, b"*", b"0", b"0", seq, b"*",
                b"NM:i:%d" % d, b"MD:Z:" + md, b"NH:i:%d" % nh[r], b"HI:i:%d" % hi, b"XM:i:%d" % nmiss]
        if count_of(tail) is not None:
            cols.append(b"XC:i:" + count_of(tail))
        out.append(b"\t".join(cols) + b"\n")
    return out


# -------------------------------------------------------------------------------------------------------------- inverse
def parse_header(hdr):
    """{SN: LN} of a header, which must be @HD, @SQ lines, @PG."""
    lines = hdr.split(b"\n")
    assert lines[-1] == b"" and lines[0] + b"\n" == HD and lines[-2] + b"\n" == PG, hdr[:80]
    ln = {}
    for line in lines[1:-2]:
        tag, sn, l = line.split(b"\t")
        assert tag == b"@SQ" and sn.startswith(b"SN:") and l.startswith(b"LN:") and sn[3:] not in ln
        ln[sn[3:]] = int(l[3:])
    return ln


def invert(hdr, record):
    """(read, targetsub, pos, gene name) of the results.txt line a record was made from, out of the header and the
    record's FLAG, RNAME, POS, CIGAR, SEQ and MD alone.  A reverse record is a line of the ``_r`` target: the read and
    the span are complemented back and the position is counted from the other end of the reference."""
    assert record.endswith(b"\n")
    f = record[:-1].split(b"\t")
    flag, rname, pos1, cigar, seq = int(f[1]), f[2], int(f[3]), f[5], f[9]
    md = [t for t in f[11:] if t.startswith(b"MD:Z:")][0][5:]
    ref_len = parse_header(hdr)[rname]
    # CIGAR -> soft clip before, aligned bases, soft clip after
    ops, num = [], b""
    for c in cigar if cigar != b"*" else b"":
        if 48 <= c <= 57:
            num += bytes([c])
        else:
            ops.append((int(num), chr(c)))
            num = b""
    assert num == b"" and [o for _, o in ops] in ([], ["M"], ["M", "S"], ["S", "M"]), cigar
    lead = ops[0][0] if ops and ops[0][1] == "S" else 0
    m = sum(n for n, o in ops if o == "M")
    bases = b"" if seq == b"*" else seq
    assert len(bases) == sum(n for n, _ in ops) or not ops
    aligned = bytearray(bases[lead:lead + m])
    # MD -> the reference under the aligned bases
    at, i = 0, 0
    while i < len(md):
        j = i
        while j < len(md) and 48 <= md[j] <= 57:
            j += 1
        assert j > i, md  # a number before and after every letter
        at += int(md[i:j])
        if j < len(md):
            assert aligned[at] != md[j], (md, at)  # a mismatch names a base the read does not have there
            aligned[at] = md[j]
            at += 1
        i = j + 1
    assert at == m, (md, cigar)
    x = lambda s: bytes(s).replace(b"N", b"X")
    if flag & 16:
        comp = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A"), ord("N"): ord("X")}
        back = lambda s: bytes(comp[c] for c in reversed(bytes(s)))
        return back(bases), back(aligned), ref_len - (pos1 - 1) - m, rname + b"_r"
    return x(bases), x(aligned), pos1 - 1, rname


# ------------------------------------------------------------------------------------------------- results.txt's order
def six_of(reads, targets, rests, h):
    r, g, p, nx = (int(v) for v in h)
    return b"\t".join([reads[r], targets[g][p:p + len(reads[r])], b"%d" % p, b"%d" % nx, rests[g]])


def ordered_hits(case):
    """The case's tuples without those of absent genes, in the line order of results.txt (ties keep any order: they are
    the same line)."""
    kept = [tuple(int(v) for v in h) for h in case.hits if int(h[1]) not in case.absent]
    return sorted(kept, key=lambda h: six_of(case.reads, case.targets, case.rests, h))


def oracle_columns(case):
    """Columns 1-3 (read, targetsub, pos) and 4 (nmiss) of the oracle's results.txt over the case's tuples."""
    ids = [b"%011d\t%s" % (g, case.rests[g]) for g in range(len(case.targets))]
    ureads = [orc.UniqueRead(r, 1, b"n") for r in case.reads]
    kept = [tuple(int(v) for v in h) for h in case.hits if int(h[1]) not in case.absent]
    txt = orc.results_text(kept, ureads, case.targets, ids, orc.Config(MMTol=KEEP_ALL))
    cols = [ln.split(b"\t") for ln in txt.split(b"\n")[:-1]]
    return [(c[0], c[1], int(c[2]), int(c[3])) for c in cols]


def sam_of(case):
    """(header, [record, ...]) of the model over a case; raises SamRefused."""
    hdr = header(case.targets, case.rests, case.absent, case.rev_pairs)
    return hdr, records(case.reads, case.targets, case.rests, case.tails, ordered_hits(case), case.rev_pairs, case.absent)


# ---------------------------------------------------------------------------------------------------------------- cases
def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def hamming(read, target, pos):
    return sum(1 for a, b in zip(read, target[pos:pos + len(read)]) if a != b)


def other(rng, c):
    return rng.choice([b for b in b"ACGT" if b != c])


class Builder:
    """Collects alignments (read sequence, gene, pos) and names; finish() sorts and numbers the reads."""

    def __init__(self, name, targets, names, rev_pairs=False, absent=()):
        self.name, self.targets, self.rev_pairs, self.absent = name, list(targets), rev_pairs, tuple(absent)
        self.rests = [b"%s\t%d" % (n, len(t)) for n, t in zip(names, targets)]
        self.al, self.tail = [], {}

    def add(self, read, g, pos, tail=None, nmiss=None):
        self.al.append((read, g, pos, hamming(read, self.targets[g], pos) if nmiss is None else nmiss))
        if tail is not None:
            self.tail[read] = tail

    def mutated(self, rng, g, pos, L, places):
        """The L bases of target g at pos with the bases at `places` replaced."""
        b = bytearray(self.targets[g][pos:pos + L])
        for p in places:
            b[p] = other(rng, b[p])
        return bytes(b)

    def finish(self, tails=True, **note):
        reads = sorted({a[0] for a in self.al})
        num = {r: i for i, r in enumerate(reads)}
        hits = sorted({(num[r], g, p, nx) for r, g, p, nx in self.al})  # (a tuple is in a list once, as in the oracle's)
        tl = [self.tail.get(r, b"%d\tq%d;z" % (1 + i % 3, i)) for i, r in enumerate(reads)] if tails else None
        return Case(self.name, reads, self.targets, self.rests, hits, tl, self.absent, self.rev_pairs, note=note)


LENS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]


def case_lengths_and_phases(max_len, seed):
    """Every length of LENS up to max_len (which fixes the stride of the read records) at spans that start at all
    sixteen phases of a database word, with 0, 1 or 2 mismatches; one target per phase offset, back to back."""
    rng = random.Random(seed)
    lens = [L for L in LENS if L <= max_len] + ([max_len] if max_len not in LENS else [])
    targets = [rand_seq(rng, 3, b"ACGT")] + [rand_seq(rng, max_len + 40 + k, b"ACGT") for k in range(3)]
    b = Builder("lengths_%d" % max_len, targets, [b"t%d" % g for g in range(len(targets))])
    starts = [0]
    for t in targets:
        starts.append(starts[-1] + len(t))
    phases = set()
    for i, L in enumerate(lens):
        for ph in range(16):
            g = 1 + (i + ph) % 3
            pos = (ph - starts[g]) % 16 + 16 * ((i + ph) % 2)
            assert pos + L <= len(targets[g])
            phases.add((starts[g] + pos) % 16)
            places = sorted(rng.sample(range(L), min(L, (i + ph) % 3)))
            b.add(b.mutated(rng, g, pos, L, places), g, pos)
    assert phases == set(range(16))
    return b.finish(lens=lens)


def case_mismatch_patterns(seed=11):
    """Mismatches at the first and the last base, adjacent ones, none, all; match runs of 9, 10, 99 and 100 before,
    between and after mismatches; on both strands."""
    rng = random.Random(seed)
    t = rand_seq(rng, 260, b"ACGT")
    targets = [t, orc.revcomp(t)]
    b = Builder("mismatch_patterns", targets, [b"chrA", b"chrA_r"], rev_pairs=True)
    pats = {
        "first": (40, [0]), "last": (40, [39]), "both_ends": (40, [0, 39]), "adjacent": (40, [10, 11, 12]),
        "none": (40, []), "all": (23, list(range(23))), "run9_10": (21, [9, 20]), "run10_9": (21, [10, 20]),
        "run99_100": (201, [99, 200]), "run100_99": (201, [100, 200]), "run100_tail": (130, [29]), "run99_tail": (130, [30]),
    }
    for k, (name, (L, places)) in enumerate(sorted(pats.items())):
        for g in (0, 1):
            pos = 3 + k + g
            b.add(b.mutated(rng, g, pos, L, places), g, pos, tail=b"%d\t%s_%d" % (k + 1, name.encode(), g))
    return b.finish(patterns=sorted(pats))


def case_x(seed=12):
    """X in the read only, in the database only, at the same place in both (no mismatch), next to each other, at the
    first and last base, and at both sides of a 16- and a 32-base word boundary; both strands."""
    rng = random.Random(seed)
    t = bytearray(rand_seq(rng, 150, b"ACGT"))
    for p in (5, 20, 31, 32, 47, 48, 64, 100):
        t[p] = ord("X")
    t = bytes(t)
    targets = [t, orc.revcomp(t)]
    b = Builder("x", targets, [b"tx", b"tx_r"], rev_pairs=True)
    for g in (0, 1):
        tg = targets[g]
        for pos, L in ((0, 70), (5, 30), (18, 40), (31, 2), (60, 45), (100, 1), (99, 3)):
            span = bytearray(tg[pos:pos + L])
            b.add(bytes(span), g, pos)                      # X at the same place in both
            plain = bytes(other(rng, c) if c == ord("X") else c for c in span)
            b.add(plain, g, pos)                            # X in the database only
            rx = bytearray(plain)
            rx[0] = rx[-1] = ord("X")
            if L > 20:
                rx[15] = rx[16] = ord("X")
            b.add(bytes(rx), g, pos)                        # X in the read (and not where the database has one, mostly)
    return b.finish()


def case_clipped(seed=13):
    """Spans clipped at the target's end (S < L) on both strands, S from 1 to L - 1, and S == 0 (pos == the target's
    length): the read hangs over the end; S == L ends exactly at it."""
    rng = random.Random(seed)
    t = rand_seq(rng, 50, b"ACGT")
    u = rand_seq(rng, 37, b"ACGT")
    targets = [t, orc.revcomp(t), u, orc.revcomp(u)]
    b = Builder("clipped", targets, [b"c1", b"c1_r", b"c2", b"c2_r"], rev_pairs=True)
    for g in range(4):
        tl = len(targets[g])
        for L, S in ((20, 20), (20, 19), (20, 1), (33, 16), (33, 17), (70, 37), (12, 0), (1, 0)):
            if S > tl:
                continue
            pos = tl - S
            read = bytearray(targets[g][pos:] + rand_seq(rng, L - S, b"ACGT"))
            if S > 2:
                read[S - 1] = other(rng, read[S - 1])  # a mismatch at the last base of the span
            b.add(bytes(read), g, pos)
    return b.finish()


def case_lines_per_read(seed=14):
    """Reads with 1, 2 and 11 lines (NH of one and two digits), some lines on genes without an id line."""
    rng = random.Random(seed)
    core = rand_seq(rng, 24, b"ACGT")
    targets = [rand_seq(rng, 3 + g, b"ACGT") + core + rand_seq(rng, 5, b"ACGT") for g in range(13)]
    b = Builder("lines_per_read", targets, [b"g%d" % g for g in range(13)], absent=(4, 12))
    for g in range(13):  # 11 present genes
        b.add(core, g, 3 + g)
    r2 = b.mutated(rng, 0, 3, 24, [7])
    b.add(r2, 0, 3)
    b.add(r2, 1, 4)
    b.add(r2, 4, 7)  # an absent gene: no line
    b.add(b.mutated(rng, 2, 5, 24, [0, 23]), 2, 5)
    b.add(rand_seq(rng, 24, b"ACGT"), 12, 0)  # a read whose only tuple is of an absent gene
    return b.finish()


def case_names(seed=15):
    """QNAME and XC: names with `;`, every whitespace byte, a leading `@` or `>` (one dropped), an empty token, 254, 255
    and 600 bytes, a tail without a tab, counts of several digits and counts that are no number; RNAME: a leading `>`,
    blanks before the name, text behind the name."""
    rng = random.Random(seed)
    t = rand_seq(rng, 60, b"ACGT")
    targets = [t, t[:50], t[5:], t[3:40]]
    b = Builder("names", targets, [b"x"] * 4)
    b.rests = [b">chr1 some text\t60", b"  \tchr2\t50", b"chr3", b">>odd\x0bname\t37"]
    tails = [b"1\tplain", b"12\tn1;n2;n3", b"1234567\t@at_name rest", b"3\t>gt_name;x", b"4\t@@two", b"5\t", b"6\t;lead",
             b"7", b"\tnocount", b"x9\tbadcount", b"9 \tblank_in_count", b"10\t" + b"A" * 254, b"11\t" + b"B" * 255,
             b"12\t" + b"C" * 600 + b";more", b"13\t@", b"14\t@;", b"007\tzeros"] + [b"2\tw" + bytes([w]) + b"after" for w in WS] + \
            [b"2\t" + bytes([w]) + b"lead" for w in WS]
    for i, tail in enumerate(tails):
        g = i % 4
        b.add(b.mutated(rng, g, i % 7, 30, [i % 30]), g, i % 7, tail=tail)
    return b.finish(tails=tails)


def case_no_read_text(seed=16):
    c = case_lines_per_read(seed)
    c.name, c.tails = "no_read_text", None
    return c


def case_rev_absent(seed=17):
    """rev_pairs with a pair that has no id lines at all (no @SQ, no records) and hits on both strands of the others."""
    rng = random.Random(seed)
    ts = [rand_seq(rng, 40 + 3 * k, b"ACGT") for k in range(3)]
    targets = [x for t in ts for x in (t, orc.revcomp(t))]
    b = Builder("rev_absent", targets, [n for k in range(3) for n in (b"p%d" % k, b"p%d_r" % k)], rev_pairs=True, absent=(2, 3))
    for g in range(6):
        for pos in (0, 7, len(targets[g]) - 25):
            b.add(b.mutated(rng, g, pos, 25, [pos % 25]), g, pos)
    return b.finish()


def refusal_cases():
    rng = random.Random(18)
    t = rand_seq(rng, 30, b"ACGT")
    rd = t[2:22]
    mk = lambda name, targets, rests, absent=(), rev=True: Case(name, [rd], targets, rests, [(0, 0, 2, 0)], [b"1\tq"], absent, rev, True)
    r = lambda n, s: b"%s\t%d" % (n, len(s))
    return [
        mk("odd_count", [t, orc.revcomp(t), t], [r(b"a", t), r(b"a_r", t), r(b"b", t)]),
        mk("unequal_pair", [t, orc.revcomp(t)[:-1]], [r(b"a", t), r(b"a_r", t[:-1])]),
        mk("empty_text", [t, orc.revcomp(t)], [b"", r(b"a_r", t)], rev=False),
        mk("only_gt", [t, orc.revcomp(t)], [b"> x\t30", r(b"a_r", t)], rev=False),
        mk("blank_text", [t, orc.revcomp(t)], [b" \t ", r(b"a_r", t)], rev=False),
        mk("even_partner_absent", [t, orc.revcomp(t)], [r(b"a", t), r(b"a_r", t)], absent=(0,)),
        mk("even_partner_empty", [t, orc.revcomp(t)], [b"", r(b"a_r", t)]),
    ]


def seeded_cases():
    return [case_lengths_and_phases(33, 1), case_lengths_and_phases(65, 2), case_lengths_and_phases(130, 3),
            case_lengths_and_phases(200, 4), case_mismatch_patterns(), case_x(), case_clipped(), case_lines_per_read(),
            case_names(), case_no_read_text(), case_rev_absent()]
