"""Coverage as the tests see it, without a GPU and without the library: a brute-force Python model --
per-base depth arrays, then runs, then both texts -- over a case of tests/sam_cases.py and the three flags, and the
seeded cases that tests/test_cov_cases.py, tests/test_gpu_cov.py and tests/test_cli_cov.py share.

A `CovCase` is a sam_cases.Case (reads distinct and sorted, targets over ACGTX, rests[g] gene g's text, absent the genes
without an id line, tails[r] read r's ``count\\tnames`` or None for no read text, hits in any order) with the flag sets
it is run under: tuples (rev_pairs, weighted, unique)."""
import random
from dataclasses import dataclass, field
from typing import List, Tuple

from oracle import muscato_oracle as orc

import sam_cases as sc

WEIGHT_LIMIT = 1 << 32
PLAIN, WEIGHTED, UNIQUE = (False, False, False), (False, True, False), (False, False, True)
REV = (True, False, False)


class CovRefused(Exception):
    """What musc_cov_prepare answers with code 12."""


@dataclass
class CovCase:
    case: sc.Case
    flagsets: List[Tuple[bool, bool, bool]]
    refused: Tuple[Tuple[bool, bool, bool], ...] = ()  # the flag sets under which the stage refuses
    note: dict = field(default_factory=dict)

    @property
    def name(self):
        return self.case.name


# ---------------------------------------------------------------------------------------------------------------- model
def weight_of(tail, weighted):
    """The weight of a line of the read with this tail (None: no read text)."""
    if not weighted or tail is None:
        return 1
    head = tail.split(b"\t", 1)[0]
    if not head or not all(48 <= c <= 57 for c in head):
        return 1
    return min(int(head), WEIGHT_LIMIT)


def interval_of(targets, g, pos, L, rev_pairs):
    """(f, a, S): the forward-strand bases [a, a + S) of target f that a line covers."""
    tl = len(targets[g])
    S = min(L, tl - pos)
    if rev_pairs and g % 2:
        return g - 1, tl - pos - S, S
    return g, pos, S


def contributions(case, ordered, rev_pairs, weighted, unique):
    """[(f, a, S, w)] of the contributing lines of `ordered`; raises CovRefused."""
    try:
        sc.check_refusals(case.targets, case.rests, case.absent, rev_pairs)
    except sc.SamRefused as e:
        raise CovRefused(str(e))
    if len(ordered) >= 1 << 31:
        raise CovRefused("2^31 lines or more")
    lines = {}
    for h in ordered:
        lines[h[0]] = lines.get(h[0], 0) + 1
    out = []
    for r, g, pos, _ in ordered:
        if unique and lines[r] != 1:
            continue
        f, a, S = interval_of(case.targets, g, pos, len(case.reads[r]), rev_pairs)
        out.append((f, a, S, weight_of(case.tails[r] if case.tails is not None else None, weighted)))
    if sum(w for _, _, _, w in out) >= WEIGHT_LIMIT:
        raise CovRefused("a total weight of 2^32 or more")
    return out


def summary_targets(case, rev_pairs):
    return [t for t in range(len(case.targets)) if t not in case.absent and not (rev_pairs and t % 2)]


def depth_arrays(case, contrib):
    depth = {}
    for f, a, S, w in contrib:
        d = depth.setdefault(f, [0] * len(case.targets[f]))
        for x in range(a, a + S):
            d[x] += w
    return depth


def runs_of(depth):
    """[(start, end, depth)] of the maximal runs of constant non-zero depth of one target's per-base array."""
    out, x, n = [], 0, len(depth)
    while x < n:
        y = x
        while y < n and depth[y] == depth[x]:
            y += 1
        if depth[x]:
            out.append((x, y, depth[x]))
        x = y
    return out


def cov_of(case, ordered, rev_pairs=False, weighted=False, unique=False):
    """([bedGraph record, ...], [summary record, ...]) of the model, every record with its newline; raises CovRefused."""
    contrib = contributions(case, ordered, rev_pairs, weighted, unique)
    depth = depth_arrays(case, contrib)
    numreads = {}
    for f, _, _, w in contrib:
        numreads[f] = numreads.get(f, 0) + w
    bed, summary = [], []
    for t in summary_targets(case, rev_pairs):
        name, d = sc.rname_of(case.rests[t]), depth.get(t, [0] * len(case.targets[t]))
        for s, e, v in runs_of(d):
            bed.append(b"%s\t%d\t%d\t%d\n" % (name, s, e, v))
        summary.append(b"%s\t%d\t%d\t%d\t%d\t%d\n" % (name, len(d), numreads.get(t, 0), sum(1 for v in d if v), sum(d), max(d, default=0)))
    assert set(depth) <= set(summary_targets(case, rev_pairs))
    return bed, summary


def cov_case_of(cc, flags):
    return cov_of(cc.case, sc.ordered_hits(cc.case), *flags)


# ---------------------------------------------------------------------------------------------------------------- cases
class Lines:
    """Collects lines (target, pos, read length, tail) over fixed targets; every line gets a read of its own."""

    def __init__(self, name, targets, names, seed, rev_pairs=False, absent=()):
        self.rng = random.Random(seed)
        self.b = sc.Builder(name, targets, names, rev_pairs=rev_pairs, absent=absent)
        self.seen = set()

    def read(self, L):
        while True:
            r = sc.rand_seq(self.rng, L, b"ACGT")
            if r not in self.seen:
                self.seen.add(r)
                return r

    def add(self, g, pos, L, tail=None, read=None):
        read = self.read(L) if read is None else read
        self.b.add(read, g, pos, tail=tail, nmiss=len(self.b.al) % 4)
        return read

    def finish(self, flagsets, tails=True, refused=(), **note):
        return CovCase(self.b.finish(tails=tails), list(flagsets), tuple(refused), note)


def _targets(rng, lens):
    return [sc.rand_seq(rng, n, b"ACGT") for n in lens]


def case_intervals():
    """Abutting intervals of equal weight (one run) and of unequal weight (two), nested and identical intervals."""
    rng = random.Random(31)
    ln = Lines("intervals", _targets(rng, [200, 200, 200, 200]), [b"abut_eq", b"abut_ne", b"nested", b"same"], 31)
    ln.add(0, 10, 20, b"3\ta"), ln.add(0, 30, 20, b"3\tb")          # [10, 30) + [30, 50), weight 3 and 3
    ln.add(1, 10, 20, b"2\tc"), ln.add(1, 30, 20, b"5\td")          # ... weight 2 and 5
    ln.add(2, 60, 40, b"1\te"), ln.add(2, 70, 10, b"4\tf")          # [70, 80) inside [60, 100)
    ln.add(3, 5, 25, b"7\tg"), ln.add(3, 5, 25, b"11\th")           # the same interval twice
    return ln.finish([PLAIN, WEIGHTED, UNIQUE])


PILES = (63, 64, 65, 255, 256, 257, 1000)


def case_piles():
    """63 ... 1 000 lines that start at one base, so that as many events share a key; the ends are spread."""
    rng = random.Random(32)
    ln = Lines("piles", _targets(rng, [120] * len(PILES)), [b"pile%d" % k for k in PILES], 32)
    for g, k in enumerate(PILES):
        for i in range(k):
            ln.add(g, 7, 12 + i % 30, b"%d\tp" % (1 + i % 3))
    return ln.finish([PLAIN, WEIGHTED], piles=PILES)


def case_target_ends():
    """An interval that ends at its target's end while the next target's starts at base 0; empty targets first, in the
    middle and last but one; uncovered targets between covered ones; the first and the last target covered; targets
    without an id line, one of them with lines."""
    rng = random.Random(33)
    lens = [40, 0, 50, 30, 0, 35, 60, 45, 0, 25]
    ln = Lines("target_ends", _targets(rng, lens), [b"e%d" % g for g in range(len(lens))], 33, absent=(5, 8))
    ln.add(0, 0, 10), ln.add(0, 20, 20)     # to the end of target 0 ...
    ln.add(2, 0, 15)                        # ... and from base 0 of the next target with bases
    ln.add(2, 35, 15), ln.add(3, 0, 30)     # likewise, with no empty target between; target 3 covered end to end
    ln.add(5, 3, 10)                        # no id line: the line vanishes
    ln.add(9, 5, 20), ln.add(9, 24, 1)      # the last target, to its last base
    return ln.finish([PLAIN, WEIGHTED], uncovered=(6, 7))


def case_strands():
    """Forward and reverse lines over the same bases of a -rev database, reverse lines with a clip, S == 0 on either
    strand; the same list without the folding."""
    rng = random.Random(34)
    ts = _targets(rng, [80, 61])
    targets = [x for t in ts for x in (t, orc.revcomp(t))]
    ln = Lines("strands", targets, [b"s0", b"s0_r", b"s1", b"s1_r"], 34, rev_pairs=True)
    ln.add(0, 10, 30, b"2\tf"), ln.add(1, 80 - 10 - 30, 30, b"3\tr")   # the same forward bases [10, 40)
    ln.add(0, 20, 30, b"1\tf2"), ln.add(1, 5, 30, b"1\tr2")            # overlapping ones
    ln.add(1, 70, 25, b"4\tclip_r"), ln.add(0, 72, 25, b"5\tclip_f")   # clipped at the target's end on either strand
    ln.add(2, 61, 12, b"6\tempty_f"), ln.add(3, 61, 12, b"7\tempty_r") # S == 0
    ln.add(3, 0, 61, b"8\twhole_r"), ln.add(2, 60, 1, b"9\tlast_f")
    return ln.finish([REV, (True, True, False), PLAIN, (True, True, True)])


def case_weights():
    """Counts 0, 1, several digits, leading zeros, no digits, empty, a tail without a tab, a tail that is only a count;
    a read with two lines."""
    rng = random.Random(35)
    ln = Lines("weights", _targets(rng, [300]), [b"w"], 35)
    tails = [b"0\tzero", b"1\tone", b"12345\tmany", b"007\tzeros", b"x9\tnodigit", b"9x\tnodigit2", b"\tempty", b"42", b"nocount", b"",
             b"5 \tblank", b"-3\tminus", b"00\tzero2"]
    for i, t in enumerate(tails):
        ln.add(0, 20 * i, 25, t)
    twice = ln.add(0, 150, 30, b"6\ttwice")
    ln.add(0, 280, 30, read=twice)
    return ln.finish([WEIGHTED, PLAIN, (False, True, True)], tail_list=tails)


def case_no_read_text():
    c = case_weights()
    c.case.name, c.case.tails = "cov_no_read_text", None
    return c


def case_total(name, counts, refused):
    """One line per count, on overlapping intervals."""
    rng = random.Random(36)
    ln = Lines(name, _targets(rng, [90]), [b"big"], 36)
    for i, n in enumerate(counts):
        ln.add(0, 5 * i, 40, b"%d\tn" % n)
    return ln.finish([WEIGHTED, PLAIN], refused=(WEIGHTED,) if refused else ())


WIDTHS = [9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000]


def case_widths():
    """Depths, starts and ends on either side of every decimal width: depths up to ten digits on a short target, starts
    and ends up to six on a target of 100 005 bases (positions past 65 535)."""
    rng = random.Random(37)
    depths = WIDTHS + [999999, 1000000, 9999999, 10000000, 99999999, 100000000, 999999999, 1000000000]
    ln = Lines("widths", _targets(rng, [100005, 20 * len(depths) + 5]), [b"long", b"deep"], 37)
    one = [ln.read(1), ln.read(1)]  # (there are four reads of one base: two of them, on many lines each)
    for i, w in enumerate(WIDTHS):
        ln.add(0, w, 1, b"%d\tw" % (2 + i % 2), read=one[i % 2])  # [9, 10) and [10, 11), ...: two runs when weighted
    ln.add(0, 65530, 10), ln.add(0, 100000, 5), ln.add(0, 99980, 9)
    for i, d in enumerate(depths):
        ln.add(1, 20 * i, 12, b"%d\td" % d)
    assert sum(depths) < WEIGHT_LIMIT
    return ln.finish([PLAIN, WEIGHTED], depths=depths)


def case_unique():
    """Reads with one, two and three lines."""
    rng = random.Random(38)
    ln = Lines("unique", _targets(rng, [100, 100, 100]), [b"u0", b"u1", b"u2"], 38)
    one = [ln.add(0, 5, 20, b"2\tone"), ln.add(1, 50, 20, b"3\tone")]
    two = ln.add(0, 10, 22, b"4\ttwo")
    ln.add(1, 10, 22, read=two)
    three = ln.add(0, 40, 24, b"5\tthree")
    ln.add(1, 45, 24, read=three), ln.add(2, 0, 24, read=three)
    return ln.finish([UNIQUE, PLAIN, (False, True, True)], one=one, two=two, three=three)


def case_list(n):
    """A list of n lines on one target of two."""
    rng = random.Random(40 + n)
    ln = Lines("list_%d" % n, _targets(rng, [400, 30]), [b"l0", b"l1"], 40 + n)
    anchor = ln.read(16)  # (a case needs a read to load; with no line it has no tuple)
    for i in range(n):
        ln.add(0, (13 * i) % 380, 10 + i % 11, b"%d\tl" % (1 + i % 4))
    c = ln.finish([PLAIN, WEIGHTED, UNIQUE])
    if n == 0:
        c.case.reads, c.case.tails = [anchor], [b"1\tanchor"]
    return c


def seeded_cases():
    out = [case_intervals(), case_piles(), case_target_ends(), case_strands(), case_weights(), case_no_read_text(),
           case_total("total_max", [WEIGHT_LIMIT - 1 - 5, 2, 3, 0], False),        # 2^32 - 1: accepted
           case_total("total_over", [WEIGHT_LIMIT - 1 - 5, 2, 3, 1], True),        # 2^32: refused
           case_total("eleven_digits", [10000000000], True),
           case_widths(), case_unique()] + [case_list(n) for n in (0, 1, 64, 65, 257)]
    # the SAM stage's cases, for the strands, the clips and the names
    by = {c.name: c for c in sc.seeded_cases()}
    for name in ("clipped", "mismatch_patterns", "x", "rev_absent"):
        out.append(CovCase(by[name], [(True, False, False), (True, True, False), (False, False, True)]))
    for name in ("lines_per_read", "names"):
        out.append(CovCase(by[name], [PLAIN, WEIGHTED, UNIQUE]))
    return out


def refusal_cases():
    """sam_cases.refusal_cases() are this stage's too (the flags: rev_pairs as the case says)."""
    return [CovCase(c, [(c.rev_pairs, False, False)], ((c.rev_pairs, False, False),)) for c in sc.refusal_cases()]
