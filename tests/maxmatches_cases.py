"""Seeded cases for the MaxMatches replay and a pure-Python model of it (no GPU).

The reference cuts a (window, key) block of muscato_confirm that holds more than MaxMatches accepted pairs in an
order-dependent way (cmd/muscato_confirm/main.go:183-244, 424-448).  `model` re-derives the blocks from every accepted
tuple (oracle match_direct without its overflow check), ranks candidates and reads by their lines and replays the cut,
as apply_maxmatches of csrc/host/muscato_host.hpp does; tests/test_maxmatches_cases.py holds it to the literal oracle,
tests/test_gpu_maxmatches.py holds the device stage to both.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field
from typing import Dict, List, Sequence, Set, Tuple

from oracle import muscato_oracle as orc

Hit = Tuple[int, int, int, int]


@dataclass
class Case:
    name: str
    reads: List[bytes]
    targets: List[bytes]
    cfg: orc.Config
    seed: int = 0


@dataclass
class Replay:
    union: Set[Hit]                      # every accepted tuple after the truncation (the literal oracle's set)
    truncated: List[Tuple[int, bytes]]   # the (window, key) blocks with more than MaxMatches pairs
    sizes: Dict[Tuple[int, bytes], int] = field(default_factory=dict)  # pairs per block, every block
    jx0_in_truncated: bool = False       # a target-start candidate sits in a truncated block
    pos_text_order: bool = False         # a truncated block orders two candidates of one gene by the TEXT of pos


def emits(h: Hit, k: int, reads: Sequence[bytes], targets: Sequence[bytes], cfg: orc.Config) -> bool:
    """Would window k's confirm emit tuple h."""
    r, g, pos, _ = h
    s, t = reads[r], targets[g]
    if not orc.window_valid(s, k, cfg):
        return False
    q1, ww = cfg.Windows[k], cfg.WindowWidth
    jx = pos + q1
    if jx + ww > len(t) or s[q1:q1 + ww] != t[jx:jx + ww]:
        return False
    if jx == 0:
        return len(s) <= min(100 - ww, len(t))
    return pos + len(s) <= len(t)


def cand_line(g: int, jx: int, k: int, targets: Sequence[bytes], cfg: orc.Config) -> bytes:
    """left \\t right \\t %011d \\t pos (cmd/muscato_screen/main.go:303-316, 341-363)."""
    t = targets[g]
    q1, ww = cfg.Windows[k], cfg.WindowWidth
    q2 = q1 + ww
    if jx == 0:
        left, right = b"", t[ww:max(min(100 - q2, len(t)), ww)]
    else:
        left = t[jx - q1:jx]
        jy = jx + ww
        right = t[jy:max(min(jy + cfg.MaxReadLength - q2, len(t)), jy)]
    return left + b"\t" + right + b"\t%011d\t%d" % (g, jx)


def read_line(s: bytes, k: int, cfg: orc.Config) -> bytes:
    q1 = cfg.Windows[k]
    return s[:q1] + b"\t" + s[q1 + cfg.WindowWidth:]


def model(reads: Sequence[bytes], targets: Sequence[bytes], cfg: orc.Config) -> Replay:
    all_hits = sorted(orc.match_direct(reads, targets, cfg, check_overflow=False))
    W, ww, MM = len(cfg.Windows), cfg.WindowWidth, cfg.MaxMatches
    blocks: Dict[Tuple[int, bytes], List[Hit]] = {}
    for h in all_hits:
        for k in range(W):
            if emits(h, k, reads, targets, cfg):
                q1 = cfg.Windows[k]
                blocks.setdefault((k, reads[h[0]][q1:q1 + ww]), []).append(h)
    rep = Replay(union=set(), truncated=[])
    kept: Dict[Tuple[int, bytes], Set[Hit]] = {}
    for bid, pairs in sorted(blocks.items()):
        rep.sizes[bid] = len(pairs)
        if len(pairs) <= MM:
            continue
        k = bid[0]
        q1 = cfg.Windows[k]
        rep.truncated.append(bid)
        pairs.sort(key=lambda h: (cand_line(h[1], h[2] + q1, k, targets, cfg), read_line(reads[h[0]], k, cfg)))
        if any(h[2] + q1 == 0 for h in pairs):
            rep.jx0_in_truncated = True
        cands = sorted({(cand_line(h[1], h[2] + q1, k, targets, cfg), h[1], h[2] + q1) for h in pairs})
        for a, b in zip(cands, cands[1:]):
            if a[1] == b[1] and a[2] > b[2] and a[0].rsplit(b"\t", 1)[0] == b[0].rsplit(b"\t", 1)[0]:
                rep.pos_text_order = True  # "10" sorts before "9"
        q: List[Hit] = []
        if cfg.MatchMode == "first":
            q = pairs[:MM + 1]
        else:
            for h in pairs:  # qinsert: append, sift up on nmiss, cut the array's tail
                q.append(h)
                i = len(q) - 1
                while i > 0:
                    j = (i - 1) // 2
                    if q[j][3] > q[i][3]:
                        q[j], q[i] = q[i], q[j]
                        i = j
                    else:
                        break
                if len(q) > MM:
                    del q[MM:]
        kept[bid] = set(q)
    for h in all_hits:
        survive = False
        for k in range(W):
            if not emits(h, k, reads, targets, cfg):
                continue
            q1 = cfg.Windows[k]
            bid = (k, reads[h[0]][q1:q1 + ww])
            if bid not in kept or h in kept[bid]:
                survive = True
                break
        if survive:
            rep.union.add(h)
    return rep


def make_case(seed: int, windows: Sequence[int], mode: str, max_matches: int) -> Case:
    """Alphabet AC (every 4-mer key is shared by many reads and target positions), 30 targets of 20-40 bases, about 25
    reads of 10-14 bases (more when MaxMatches is large, so that blocks still overflow), window width 4.  Planted: a
    homopolymer target and read (candidates of one gene whose lines differ only in pos, 9 against 10 among them),
    reads cut from target starts (jx == 0), an X in targets and in reads inside and outside a window; the reads are
    shuffled (the ABI does not ask for sorted reads)."""
    rng = random.Random(seed * 1000 + max_matches * 7 + len(windows) + (mode == "first"))
    alpha = b"AC"
    rnd = lambda n: bytes(rng.choice(alpha) for _ in range(n))
    targets = [rnd(rng.randint(20, 40)) for _ in range(29)] + [b"A" * 40]
    for g in (3, 11):  # a database with X: X == X keys and flanks with X
        t = bytearray(targets[g])
        t[rng.randrange(2, len(t) - 2)] = ord("X")
        targets[g] = bytes(t)
    nreads = 25 if max_matches <= 6 else 70
    reads = set()
    while len(reads) < nreads:
        c = rng.random()
        L = rng.randint(10, 14)
        if c < 0.5:
            t = targets[rng.randrange(len(targets))]
            p = rng.randrange(len(t) - L + 1)
            r = bytearray(t[p:p + L])
            if rng.random() < 0.4:
                j = rng.randrange(L)
                r[j] = alpha[1 - alpha.index(r[j])] if r[j] in alpha else alpha[0]
            reads.add(bytes(r))
        elif c < 0.65:
            reads.add(targets[rng.randrange(len(targets))][:L])  # a target's start
        else:
            reads.add(rnd(L))
    reads.add(b"A" * 12)
    r = bytearray(rnd(12))
    r[1] = ord("X")  # an X inside window 0
    reads.add(bytes(r))
    r = bytearray(targets[3][:12]) if len(targets[3]) >= 12 else bytearray(rnd(12))
    reads.add(bytes(r))
    r = bytearray(rnd(13))
    r[4] = ord("X")  # outside windows [0,4) and [5,9)
    reads.add(bytes(r))
    reads = sorted(reads)
    rng.shuffle(reads)
    cfg = orc.Config(Windows=list(windows), WindowWidth=4, PMatch=0.7, MinDinuc=0, MaxReadLength=14,
                     MaxMatches=max_matches, MMTol=1, MatchMode=mode)
    return Case("s%d-w%s-%s-mm%d" % (seed, "".join(map(str, windows)), mode, max_matches), reads, targets, cfg, seed)


def long_case(mode: str) -> Case:
    """100-base reads on 300-base targets over ACGT, windows [0, 20] of 15 bases: a 160-base motif sits in 25 of 40 genes,
    and 14 reads are cut from it, so that their blocks hold far more than MaxMatches = 20 pairs whose candidates have
    flanks that agree for 32 bases and more.  Some copies differ from the motif deep in the right flank (a substitution,
    an X), some sit at the target's start or flush with its end (short flanks, jx == 0)."""
    rng = random.Random(160 + (mode == "first"))
    rnd = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    motif = rnd(160)
    targets = []
    for g in range(40):
        t = bytearray(rnd(300))
        if g < 25:
            p = 0 if g == 0 else 140 if g == 1 else rng.randrange(1, 140)
            m = bytearray(motif)
            if g % 5 == 2:
                j = rng.randrange(60, 150)
                m[j] = b"ACGT"[(b"ACGT".index(m[j]) + 1) % 4]
            if g % 7 == 3:
                m[rng.randrange(70, 150)] = ord("X")
            t[p:p + 160] = m
        targets.append(bytes(t))
    reads = {motif[o:o + L] for o, L in ((0, 100), (0, 85), (0, 60), (8, 100), (8, 90), (16, 100), (16, 70), (24, 100),
                                         (24, 100 - 9), (32, 100), (40, 100), (48, 100), (56, 100), (60, 100))}
    r = bytearray(motif[8:108])
    r[90] = ord("X")
    reads.add(bytes(r))
    while len(reads) < 24:
        t = targets[rng.randrange(25, 40)]
        L = rng.randint(40, 100)
        p = rng.randrange(300 - L + 1)
        reads.add(t[p:p + L])
    reads = sorted(reads)
    rng.shuffle(reads)
    cfg = orc.Config(Windows=[0, 20], WindowWidth=15, PMatch=0.95, MinDinuc=2, MaxReadLength=100, MaxMatches=20, MMTol=1,
                     MatchMode=mode)
    return Case("long-" + mode, reads, targets, cfg, 160)


# (seed, windows, mode, MaxMatches): both window sets, both modes, MaxMatches around 1 and around the wave width
CASE_PARAMS = [
    (1, (0, 5), "best", 1), (1, (0, 3, 6), "first", 1),
    (2, (0, 5), "first", 2), (2, (0, 3, 6), "best", 2),
    (3, (0, 5), "best", 3), (3, (0, 3, 6), "first", 3),
    (4, (0, 5), "first", 6), (4, (0, 3, 6), "best", 6), (5, (0, 5), "best", 6),
    (6, (0, 5), "best", 63), (6, (0, 3, 6), "first", 63),
    (7, (0, 5), "first", 64), (7, (0, 3, 6), "best", 64),
    (8, (0, 5), "best", 65), (8, (0, 3, 6), "first", 65),
]


def cases() -> List[Case]:
    return [make_case(*p) for p in CASE_PARAMS] + [long_case("best"), long_case("first")]
