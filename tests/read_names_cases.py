"""Seeded FASTQ texts for the read-name stage and a pure-Python model of it in its parallel form.

The model computes what the stage has to compute the way kernels would: a clipped length and a token
length per name, the bytes of a clipped name by position (the dots are virtual), the order within a group by comparing
8-byte big-endian words (rank by counting in groups of up to 64, a comparison sort above), offsets by scanning
token + 1, and the bytes of a join by position under the cut at 996.  It counts the branches it takes (`cover`), so that
tests/test_read_names_cases.py can assert that each case reaches what it is there for; that file holds the model to
fastq_cases.unique / join_names and to the oracle.  A device stage is to be held to the model, byte for byte."""
import functools
import random
from dataclasses import dataclass, field
from typing import List

import fastq_cases as fc

NAME_LIMIT, NAME_KEEP, JOIN_LIMIT, JOIN_KEEP, DOTS, WAVE_GROUP_MAX = 1000, 995, 1000, 996, 3, 64


# ---- the size rules (read_names_plan.hpp)
def text_len(n):
    return NAME_KEEP if n > NAME_LIMIT else n


def clipped_len(n):
    return NAME_KEEP + DOTS if n > NAME_LIMIT else n


def virtual_byte(n, i):
    return n > NAME_LIMIT and i >= NAME_KEEP


def token_len(name: bytes):
    tl = text_len(len(name))
    tab = name.find(b"\t", 0, tl)
    return tab if tab >= 0 else clipped_len(len(name))


def dec_width(v):
    return len(str(v))


def group_path(count):
    return "single" if count <= 1 else "wave" if count <= WAVE_GROUP_MAX else "sorted"


def name_byte(name: bytes, i: int) -> int:
    return 0x2E if virtual_byte(len(name), i) else name[i]


def name_word(name: bytes, w: int) -> int:
    """Bytes [8 w, 8 w + 8) of the clipped name, the first most significant, 0 past its end."""
    cl, v = clipped_len(len(name)), 0
    for i in range(8 * w, 8 * w + 8):
        v = v << 8 | (name_byte(name, i) if i < cl else 0)
    return v


@dataclass
class NamesModel:
    prep: fc.Model = None
    seqs: List[bytes] = field(default_factory=list)      # the distinct prepared reads, in order
    counts: List[int] = field(default_factory=list)
    members: List[List[int]] = field(default_factory=list)  # per group: kept-read numbers in ranked order
    records: List[bytes] = field(default_factory=list)   # count \t J
    lines: List[bytes] = field(default_factory=list)     # seq \t count \t J \n
    info: dict = field(default_factory=dict)
    cover: set = field(default_factory=set)

    @property
    def text(self):
        return b"".join(self.records)

    @property
    def line_text(self):
        return b"".join(self.lines)


def compare(a: bytes, b: bytes, cover: set, off_a: int = 0) -> int:
    """The order of two clipped names, word by word; what decided goes into `cover`."""
    ca, cb = clipped_len(len(a)), clipped_len(len(b))
    for w in range((min(ca, cb) + 7) // 8):
        x, y = name_word(a, w), name_word(b, w)
        if x != y:
            p = 8 * w + (7 - ((x ^ y).bit_length() - 1) // 8)  # the first byte that differs
            cover.add("diff:%d" % p)
            cover.add("phase:%d:%d" % (p, (off_a + 8 * w) % 8))
            if p >= min(ca, cb):
                cover.add("prefix_in_word")
            else:
                cover.add("bytes:%02x:%02x" % tuple(sorted((name_byte(a, p), name_byte(b, p)))))
            return -1 if x < y else 1
    if ca != cb:
        cover.add("prefix")
        return -1 if ca < cb else 1
    cover.add("equal_clipped" if a != b else "equal")
    if a != b and a[:NAME_KEEP] == b[:NAME_KEEP]:
        d = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
        cover.add("tie_beyond:%d" % d)
    return 0


def model(raw: bytes, min_len: int, max_len: int) -> NamesModel:
    m = NamesModel(prep=fc.model(raw, min_len, max_len))
    P, cover = m.prep, m.cover
    clip = [clipped_len(len(n)) for n in P.names]
    tok = [token_len(n) for n in P.names]
    for n, off in zip(P.names, P.name_off):
        cover.add("len:%d" % len(n))
        cover.add("align:%d" % (off % 16))
        tl = text_len(len(n))
        tabs = [i for i in range(len(n)) if n[i] == 9]
        cover.add("tabs:%d" % min(len(tabs), 2))
        if tabs:
            cover.add("tab_first" if tabs[0] == 0 else "tab_last" if tabs[0] == len(n) - 1 else "tab_mid")
            if len(n) > NAME_LIMIT:
                cover.add("long_tab:%d:%s" % (tabs[0], "cut_away" if tabs[0] >= tl else "kept"))
    groups = {}
    for i, s in enumerate(P.seqs):
        groups.setdefault(s, []).append(i)  # file order
    info = dict(n_unique=len(groups), n_single=0, n_wave_groups=0, n_sorted_groups=0, n_clipped_joins=0,
                n_clipped_names=sum(len(n) > NAME_LIMIT for n in P.names), max_group=max([len(g) for g in groups.values()] + [0]))
    for s in sorted(groups):
        g = groups[s]
        k = len(g)
        path = group_path(k)
        cover.add("path:" + path)
        cover.add("group:%d" % k)
        cover.add("digits:%d" % dec_width(k))
        info["n_single" if path == "single" else "n_wave_groups" if path == "wave" else "n_sorted_groups"] += 1
        # ---- rank
        if path == "single":
            ranked = list(g)
        elif path == "wave":  # member i counts the names in front of its own, equal names in file order
            ranked = [None] * k
            for i in range(k):
                r = 0
                for o in range(k):
                    if o != i:
                        d = compare(P.names[g[o]], P.names[g[i]], cover, P.name_off[g[o]])
                        r += d < 0 or (d == 0 and o < i)
                ranked[r] = g[i]
        else:
            ranked = sorted(g, key=functools.cmp_to_key(
                lambda x, y: compare(P.names[x], P.names[y], cover, P.name_off[x]) or (x > y) - (x < y)))
        if ranked != g:
            cover.add("reordered")
        # ---- offsets by scan, bytes by position
        starts, base = [], 0
        for r in ranked:
            starts.append(base)
            base += tok[r] + 1
        total = base - 1
        clipped = total > JOIN_LIMIT
        limit = JOIN_KEEP if clipped else total
        J = bytearray(limit + (DOTS if clipped else 0))
        for j, r in enumerate(ranked):
            if starts[j] >= limit:
                break
            for p in range(tok[r]):
                if starts[j] + p < limit:
                    J[starts[j] + p] = name_byte(P.names[r], p)
            if j + 1 < k and starts[j] + tok[r] < limit:
                J[starts[j] + tok[r]] = 0x3B
        if clipped:
            J[limit:] = b"..."
            info["n_clipped_joins"] += 1
            cover.add("overflow:" + path)
            seps = set(st - 1 for st in starts[1:])
            cover.add("cut:on_sep" if JOIN_KEEP in seps else "cut:after_sep" if JOIN_KEEP - 1 in seps else "cut:mid")
            if tok[ranked[0]] == NAME_KEEP + DOTS:
                cover.add("first_998")
        if total >= JOIN_LIMIT - 1:
            cover.add("join:%d" % min(total, JOIN_LIMIT + 3))
        if b";;" in J:
            cover.add("empty_token_inside")
        m.seqs.append(s)
        m.counts.append(k)
        m.members.append(ranked)
        rec = b"%d\t%s" % (k, bytes(J))
        m.records.append(rec)
        m.lines.append(s + b"\t" + rec + b"\n")
    info["n_text_bytes"] = sum(len(r) for r in m.records)
    info["n_line_bytes"] = sum(len(r) for r in m.lines)
    m.info = info
    return m


# ---- the texts
@dataclass
class Case:
    name: str
    raw: bytes
    min_len: int
    max_len: int
    covers: tuple  # entries of the model's `cover` this case is there for


class Text:
    """Records of distinct groups; every group can be put at a chosen alignment by a filler record in front of it."""

    def __init__(self):
        self.raw, self.k = b"", 0

    def seq(self):
        self.k += 1
        return bytes(b"ACGT"[(self.k >> (2 * j)) & 3] for j in range(12)) + b"GATTACA"

    def rec(self, name: bytes, seq: bytes):
        self.raw += name + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n"

    def group(self, names, align=None):
        if align is not None:  # the first name of the group starts at `align` modulo 16
            fill = self.seq()
            fixed = 1 + len(fill) + 3 + len(fill) + 1
            pad = (align - (len(self.raw) + fixed)) % 16
            self.rec(b"f" * pad, fill)
            assert len(self.raw) % 16 == align
        s = self.seq()
        for n in names:
            self.rec(n, s)


def long_name(rng, n, head=b"@L"):
    return head + bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789_/:") for _ in range(n - len(head)))


def _name_cases():
    rng = random.Random(2300)
    out = []
    lens = (0, 1, 7, 8, 9, 994, 995, 996, 997, 998, 999, 1000, 1001, 1100)
    t = Text()
    for i, n in enumerate(lens):
        t.group([long_name(rng, n) if n >= 2 else b"@"[:n]], align=(3 * i) % 16)
    t.group([long_name(rng, n) if n >= 2 else b"@"[:n] for n in reversed(lens)], align=5)
    out.append(Case("lengths", t.raw, 1, 100, tuple("len:%d" % n for n in lens) + ("path:single", "path:wave", "overflow:wave")))

    t = Text()  # pairs that first differ at byte d, the greater one first in the file, at every alignment
    for d in range(17):
        for a in range(16):
            stem = long_name(rng, d + 6)
            lo, hi = stem[:d] + b"A" + stem[d + 1:], stem[:d] + b"b" + stem[d + 1:]
            t.group([hi, lo], align=a)
    out.append(Case("pairs_diff", t.raw, 1, 100, tuple("diff:%d" % d for d in range(17)) +
                    tuple("phase:%d:%d" % (d, a) for d in range(17) for a in range(8)) +
                    tuple("align:%d" % a for a in range(16)) + ("reordered",)))

    t = Text()  # names over 1000 bytes: a difference up to byte 994 orders them, one beyond does not
    for i, d in enumerate((993, 994, 995, 996, 997)):
        stem = long_name(rng, 1010)
        t.group([stem[:d] + b"z" + stem[d + 1:], stem[:d] + b"B" + stem[d + 1:], stem[:d] + b"k" + stem[d + 1:]], align=(5 * i + 1) % 16)
    stem = long_name(rng, 1005)
    t.group([stem, stem[:995] + b"...", stem[:995] + b"..", stem[:995] + b"...."], align=7)  # 998 bytes that end in dots beside the clipped one
    t.group([b"@prefix_and_more", b"@prefix", b"@prefix_and", b"@prefix_", b"@prefix_a"], align=2)
    out.append(Case("long_and_prefix", t.raw, 1, 100, ("diff:993", "diff:994", "tie_beyond:995", "tie_beyond:996", "tie_beyond:997",
                                                      "equal_clipped", "prefix", "prefix_in_word", "reordered", "len:998")))

    t = Text()  # unsigned bytes: a signed compare puts 0x80 and 0xFF in front of 0x00 and 0x7F
    for i, (x, y) in enumerate(((0x00, 0x7F), (0x7F, 0x80), (0x80, 0xFF), (0x00, 0xFF), (0x00, 0x80), (0x7F, 0xFF))):
        for d in (0, 3, 7, 8, 13):
            stem = long_name(rng, 15)
            t.group([stem[:d] + bytes([y]) + stem[d + 1:], stem[:d] + bytes([x]) + stem[d + 1:]], align=(i + d) % 16)
    out.append(Case("high_bytes", t.raw, 1, 100, ("bytes:00:7f", "bytes:7f:80", "bytes:80:ff", "bytes:00:ff", "bytes:00:80", "bytes:7f:ff",
                                                 "reordered")))

    t = Text()
    ln = long_name(rng, 1100)
    t.group([b"\tlead", b"@z\tlate", b"@last\t"], align=9)
    t.group([ln[:994] + b"\t" + ln[995:]], align=1)
    t.group([ln[:995] + b"\t" + ln[996:]], align=12)
    t.group([b"@two\ttabs\there", b"@none"], align=4)
    t.group([b"", b"\tq", b""], align=15)  # three empty tokens: ;;
    t.group([b"@m", b"", b"@a"], align=6)
    out.append(Case("tabs", t.raw, 1, 100, ("tab_first", "tab_last", "tab_mid", "tabs:0", "tabs:1", "tabs:2", "long_tab:994:kept",
                                           "long_tab:995:cut_away", "len:0", "empty_token_inside")))
    return out


def _group_cases():
    out = []
    t = Text()
    sizes = (1, 2, 3, 63, 64, 65, 256, 257)
    for i, k in enumerate(sizes):  # names in reverse file order: the identity permutation fails
        t.group([b"@g%d_%04d" % (k, j) for j in reversed(range(k))], align=(7 * i) % 16)
    out.append(Case("group_sizes", t.raw, 1, 100, tuple("group:%d" % k for k in sizes) +
                    ("path:single", "path:wave", "path:sorted", "reordered", "overflow:sorted")))
    t = Text()
    t.group([b"@r%04d" % j for j in reversed(range(5000))], align=3)
    out.append(Case("group_5000", t.raw, 1, 100, ("group:5000", "path:sorted", "overflow:sorted", "digits:4", "reordered")))
    t = Text()
    counts = (9, 10, 99, 100, 999, 1000)
    for i, k in enumerate(counts):
        t.group([b"@c%d" % ((j * 7919) % k) for j in range(k)], align=(3 * i + 2) % 16)
    t.group([b""] * 1000, align=0)  # 999 separators and nothing else: the longest join that is not clipped
    out.append(Case("counts", t.raw, 1, 100, tuple("group:%d" % k for k in counts) + ("digits:1", "digits:2", "digits:3", "digits:4",
                                                                                    "join:999", "equal")))
    return out


def _join_cases():
    rng = random.Random(2301)
    out = []
    t = Text()
    for i, total in enumerate((999, 1000, 1001, 1002)):  # four tokens and three ';'
        last = total - 3 - 3 * 249
        t.group([long_name(rng, n, b"@j%d" % j) for j, n in enumerate((249, last, 249, 249))], align=(5 * i) % 16)
    out.append(Case("join_lengths", t.raw, 1, 100, ("join:999", "join:1000", "join:1001", "join:1002", "cut:mid")))
    t = Text()
    # (the names sort by their heads @0 @1 @2) a ';' at byte 996; a ';' at byte 995; the cut inside a token, by a wave and by the sort
    t.group([long_name(rng, 498, b"@1"), long_name(rng, 497, b"@0"), long_name(rng, 30, b"@2")], align=11)
    t.group([long_name(rng, 497, b"@1"), long_name(rng, 497, b"@0"), long_name(rng, 30, b"@2")], align=14)
    t.group([long_name(rng, 60, b"@w%02d" % j) for j in reversed(range(40))], align=8)
    t.group([long_name(rng, 30, b"@s%03d" % j) for j in reversed(range(100))], align=13)
    out.append(Case("join_cuts", t.raw, 1, 100, ("cut:on_sep", "cut:after_sep", "cut:mid", "overflow:wave", "overflow:sorted")))
    t = Text()
    t.group([b"@r%04d" % j for j in reversed(range(4999))] + [long_name(rng, 998, b"@!")], align=10)
    out.append(Case("first_998", t.raw, 1, 100, ("group:5000", "first_998", "overflow:sorted")))
    return out


_CASES = None


def cases() -> List[Case]:
    global _CASES
    if _CASES is None:
        own = _name_cases() + _group_cases() + _join_cases()
        whole = [Case("fq_" + c.name, c.raw, c.min_len, c.max_len, ()) for c in fc.cases()]
        _CASES = own + whole
    return _CASES


_MODELS = {}


def model_of(c: Case) -> NamesModel:
    """Computed once per case and shared; nobody changes it."""
    if c.name not in _MODELS:
        _MODELS[c.name] = model(c.raw, c.min_len, c.max_len)
    return _MODELS[c.name]
