"""The fixtures of the counter tests (tests/test_stats_model.py checks them on the model alone, tests/test_gpu_stats.py
runs them): a database small enough for the plain-Python model and dense enough that, at WindowWidth 6, every table is
direct by the documented rules (4^6 = 4096 buckets against about 25 000 window starts: six entries per bucket, so most
probes walk overflow entries and a few buckets stay empty), and read sets that reach every term of the counters."""
import numpy as np

from oracle import literal
from oracle import muscato_oracle as orc

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
WW = 6
MOTIF_LEN = 120
MOTIF_COPIES = 30


def _database(seed=41, n=64):
    """64 targets of 200-600 random bases; the last 12 are copies of earlier ones with 2 % substitutions (reads
    multi-map); one 120-base motif sits in 30 of the others (a read cut from it has 30 placements, and its window
    keys fill their buckets well past the inline entries)."""
    rng = np.random.default_rng(seed)
    T = [BASES[rng.integers(0, 4, size=int(rng.integers(200, 601)))] for _ in range(n)]
    ncopy = 12
    for i in range(n - ncopy, n):
        t = T[int(rng.integers(0, n - ncopy))].copy()
        sub = rng.random(len(t)) < 0.02
        t[sub] = BASES[rng.integers(0, 4, size=int(sub.sum()))]
        T[i] = t
    motif = BASES[rng.integers(0, 4, size=MOTIF_LEN)]
    for i in rng.choice(n - ncopy, size=MOTIF_COPIES, replace=False):
        p = int(rng.integers(0, len(T[i]) - MOTIF_LEN + 1))
        T[i][p:p + MOTIF_LEN] = motif
    return [bytes(t) for t in T], bytes(motif)


TARGETS, MOTIF = _database()
NBASES = sum(map(len, TARGETS))


def database_with_x(seed=43):
    """TARGETS with one X in every fifth target and a run of three in every eleventh (an entry whose context lists
    one, two, or "several" X)."""
    rng = np.random.default_rng(seed)
    out = []
    for i, t in enumerate(TARGETS):
        b = bytearray(t)
        if i % 5 == 0:
            b[int(rng.integers(0, len(b)))] = ord("X")
        if i % 11 == 0:
            p = int(rng.integers(0, len(b) - 3))
            b[p:p + 3] = b"XXX"
        out.append(bytes(b))
    return out


def mutate(rng, s, rate):
    a = np.frombuffer(s, dtype=np.uint8).copy()
    sub = rng.random(len(a)) < rate
    a[sub] = BASES[rng.integers(0, 4, size=int(sub.sum()))]
    return bytes(a)


def _finish(out):
    reads = sorted(out)
    if len(reads) % 64 == 0:
        reads = reads[:-1]
    return reads


def ragged_reads(seed=1, n=3000, max_len=100, targets=None):
    """Ragged reads, sorted and unique, their count no multiple of 64: shorter than the first window's end (3-5
    bases) and than the later windows' ends; low-complexity ones (one base, a dinucleotide repeat: fewer distinct
    dinucleotides than MinDinuc 3 in every window); cut from a target at position 0 (those of more than 94 bases
    meet the literal-100 rule at jx = 0), flush with a target end, or anywhere, with 2 % substitutions; cut from the
    motif (30 placements each); random."""
    rng = np.random.default_rng(seed)
    targets = TARGETS if targets is None else targets
    out = set()
    while len(out) < n:
        u = rng.random()
        L = int(rng.choice(np.r_[np.arange(3, 26), np.arange(26, max_len - 6), [max_len - 5] * 5, np.arange(max_len - 5, max_len + 1), [max_len] * 30]))
        if u < 0.03:
            out.add(bytes([b"ACGT"[int(rng.integers(0, 4))]]) * L)
        elif u < 0.06:
            out.add((bytes(BASES[rng.integers(0, 4, size=2)]) * L)[:L])
        elif u < 0.18:
            out.add(bytes(BASES[rng.integers(0, 4, size=L)]))
        elif u < 0.26 and L <= MOTIF_LEN:
            o = int(rng.integers(0, MOTIF_LEN - L + 1))
            out.add(mutate(rng, MOTIF[o:o + L], 0.02))
        else:
            t = targets[int(rng.integers(0, len(targets)))]
            v = rng.random()
            p = 0 if v < 0.15 else len(t) - L if v < 0.3 else int(rng.integers(0, len(t) - L + 1))
            out.add(mutate(rng, t[p:p + L], 0.02))
    return _finish(out)


def heavy_reads(seed=2, n=300, extra=250):
    """Reads of 60-100 bases from the motif, 1 % substitutions: about 30 tuples each, many more candidates, among
    `extra` ragged ones (every kind of window and candidate the counters tell apart is there).  As the
    FIRST read set of a fresh context, more tuples and descriptors per read than the first pass provides for: it must
    grow its staging / descriptor space and repeat a batch."""
    rng = np.random.default_rng(seed)
    out = set()
    while len(out) < n:
        L = int(rng.integers(60, 101))
        o = int(rng.integers(0, MOTIF_LEN - L + 1))
        out.add(mutate(rng, MOTIF[o:o + L], 0.01))
    return _finish(out | set(ragged_reads(seed + 100, extra)))


def fixed_reads(seed=3, n=2500, L=100):
    """Reads of exactly L bases (the streamed load takes one length only): from the targets, the motif, random."""
    rng = np.random.default_rng(seed)
    out = set()
    while len(out) < n:
        u = rng.random()
        if u < 0.15:
            out.add(bytes(BASES[rng.integers(0, 4, size=L)]))
        elif u < 0.25:
            o = int(rng.integers(0, MOTIF_LEN - L + 1))
            out.add(mutate(rng, MOTIF[o:o + L], 0.02))
        else:
            t = TARGETS[int(rng.integers(0, len(TARGETS)))]
            v = rng.random()
            p = 0 if v < 0.1 else len(t) - L if v < 0.2 else int(rng.integers(0, len(t) - L + 1))
            out.add(mutate(rng, t[p:p + L], 0.02))
    return _finish(out)


def reads_with_x(seed=4, n=1500):
    """ragged_reads with one X in a third of the reads of 30 bases and more -- inside a window for some, outside every
    window for others."""
    rng = np.random.default_rng(seed)
    out = set()
    for r in ragged_reads(seed, n):
        b = bytearray(r)
        if len(b) >= 30 and rng.random() < 0.33:
            b[int(rng.integers(0, len(b)))] = ord("X")
        out.add(bytes(b))
    return _finish(out)


def cfg(windows, **kw):
    c = dict(Windows=list(windows), WindowWidth=WW, PMatch=0.95, MinDinuc=3, MaxReadLength=100, MaxMatches=1000000, MMTol=1)
    c.update(kw)
    return orc.Config(**c)


# The paths of the GPU module: name -> (environment, the model's index kind, Windows).  Three windows on wide buckets
# (0,20,40 with 100-base reads: 140 bases of context); four windows 0,6,13,20 within the narrow buckets' 120.
PATHS = {
    "t1": ({}, "ctx", (0,)),
    "t2": ({}, "ctx", (0, 20)),
    "t4": ({}, "ctx", (0, 6, 13, 20)),
    "wide3": ({"MUSC_CONTEXT": "wide"}, "ctx_wide", (0, 20, 40)),
    "dma": ({"MUSC_MATCH": "dma"}, "ctx", (0, 20)),
    "c64_1": ({"MUSC_INDEX": "classic64"}, "classic64", (0,)),
    "c64_2": ({"MUSC_INDEX": "classic64"}, "classic64", (0, 20)),
    "lines_t": ({"MUSC_INDEX": "lines"}, "lines", (0, 20)),
    "lines_wg": ({"MUSC_INDEX": "lines", "MUSC_SCREEN": "wg"}, "lines", (0, 20)),
}

_FULL = {}


def oracle_full(reads, targets, c):
    """Every accepted tuple, sorted uint32 [n, 4]: oracle/literal.cpp with MaxMatches out of the way (what
    orc.match_direct(..., check_overflow=False) returns).  Cached per (reads, targets, parameters)."""
    key = (id(reads), id(targets), tuple(c.Windows), c.WindowWidth, c.PMatch, c.MinDinuc)
    if key not in _FULL:
        gbuf, goff = literal.concat(targets)
        rbuf, roff = literal.concat(reads)
        big = orc.Config(**dict(c.__dict__, MaxMatches=2 ** 31 - 1))
        full, _, _ = literal.match_arrays(rbuf, roff, gbuf, goff, literal.make_params(big, bloom_size=4_000_000, num_hash=8, nthreads=4))
        _FULL[key] = (full, reads, targets)  # (the lists are kept: their ids stay theirs)
    return _FULL[key][0]


_SETS = {}


def read_set(name):
    """The named read set, built once: "ragged", "heavy", "fixed", "x"."""
    if name not in _SETS:
        _SETS[name] = {"ragged": ragged_reads, "heavy": heavy_reads, "fixed": fixed_reads, "x": reads_with_x}[name]()
    return _SETS[name]


_EXP = {}


def expected_for(path, rs, apply_mmtol=False, parts=None, targets=None, **kw):
    """-> (oracle Config, reads, every accepted tuple, the model's counters) of read set `rs` on path `path` (a key of
    PATHS), computed once per argument set.  targets: another database than TARGETS (kept by the caller)."""
    from stats_model import expected
    _, kind, windows = PATHS[path]
    c = cfg(windows, **kw)
    reads = read_set(rs)
    tg = TARGETS if targets is None else targets
    full = oracle_full(reads, tg, c)
    key = (kind, windows, rs, apply_mmtol, tuple(parts) if parts else None, id(tg), tuple(sorted(kw.items())))
    if key not in _EXP:
        _EXP[key] = (expected(reads, tg, c, kind, full, parts=parts, apply_mmtol=apply_mmtol), tg)
    return c, reads, full, _EXP[key][0]
