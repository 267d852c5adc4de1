"""Inputs and expected text of the loader readback tests (tests/test_gpu_loaders.py), in plain Python and numpy.

The readback: musc_results_order on a hand-fed tuple list followed by musc_results_text renders, per tuple, the read from
the 2-bit records and target[pos : pos + len(read)] from the database planes -- so the text of well-chosen tuples is
the loaded data, base for base.  This module makes the seeded inputs (every set comes with the coverage condition that
tests/test_loader_cases.py asserts without a GPU), says what the text must be (expected_lines) and packs bases into the
ABI's packed form with a loop that shares nothing with muscato_amd.api.pack_2bit (ref_pack)."""
import functools
import random

import numpy as np

ACGT = b"ACGT"
_XTAB = bytes(c if c in ACGT else ord("X") for c in range(256))

# the longest read of each ragged set: the last length of record strides 4, 8, 12, 16, the first of 8, 12, 16, 20, and a
# long record of a stride no kernel is specialised for
RAGGED_MAXLENS = (48, 49, 112, 113, 176, 177, 240, 241, 1000)
RAGGED_STRIDES = (4, 8, 8, 12, 12, 16, 16, 20, 64)
N_RAGGED = 300
X_PLACES = (0, 15, 16, 31, 32)  # and the last base

FIXED_LENS = (1, 3, 15, 16, 17, 31, 33, 37, 63, 64, 65, 90, 101, 151, 250)
N_FIXED = 1000  # not a multiple of 64: the last piece of a streamed upload is ragged

TARGET_LENS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 257)  # and the empty target, three times
DB_X_BASES = (15, 16, 63, 64, 2047, 2048)  # word and X-block boundaries of the database planes
ODD_BYTES = (b"N", b"n", b"a", b"-", b"\x00", b"\xff")  # each once in the X database: all of them read as X


def record_words(maxlen):
    """The library's record stride for reads of at most maxlen bases: roundup4((2 maxlen + 31) / 32 + 1), at least 4."""
    return max(4, ((2 * maxlen + 31) // 32 + 1 + 3) & ~3)


def as_x(seq):
    """Every byte outside ACGT as X: how the loaders read a sequence."""
    return bytes(seq).translate(_XTAB)


def rand_bases(rng, n):
    return bytes(rng.choice(ACGT) for _ in range(n))


def expected_lines(reads, targets, rests, hits):
    """One `read \\t span \\t pos \\t nmiss \\t rest \\n` per tuple (read, gene, pos, nmiss), in the tuples' order; span =
    target[pos : pos + len(read)], clipped at the target's end; every byte outside ACGT written as X."""
    out = []
    for r, g, p, nx in hits:
        read = reads[r]
        out.append(b"%s\t%s\t%d\t%d\t%s\n" % (as_x(read), as_x(targets[g][p:p + len(read)]), p, nx, rests[g]))
    return out


def ref_pack(seq, garbage=None):
    """`seq` (ASCII bases, back to back) in the ABI's packed form, one base at a time: 2 bits a base (A0 C1 G2 T3), base j
    in bits [2j % 8, 2j % 8 + 2) of byte j / 4, and the mask, bit j % 8 of byte j / 8 set where the base is none of ACGT.
    garbage: a random.Random -- the code under a set mask bit is a random non-zero one (the ABI says it is ignored),
    else 0.  -> (bases uint8, mask uint8, number of X); both arrays end with 16 spare zero bytes."""
    n = len(seq)
    b2 = bytearray((n + 3) // 4 + 16)
    bm = bytearray((n + 7) // 8 + 16)
    nx = 0
    for j in range(n):
        code = ACGT.find(seq[j:j + 1])
        if code < 0:
            nx += 1
            bm[j >> 3] |= 1 << (j & 7)
            code = garbage.randint(1, 3) if garbage is not None else 0
        b2[j >> 2] |= code << (2 * (j & 3))
    return np.frombuffer(bytes(b2), dtype=np.uint8).copy(), np.frombuffer(bytes(bm), dtype=np.uint8).copy(), nx


def offsets_of(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if len(seqs):
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return off


def has_x(seq):
    return as_x(seq) != bytes(seq) or b"X" in seq


def _put_x(rng, read, places):
    b = bytearray(read)
    for p in places:
        b[p] = ord("X")
    return bytes(b)


@functools.lru_cache(maxsize=None)
def ragged_reads(maxlen, with_x):
    """N_RAGGED reads back to back in shuffled order: every length 0..min(maxlen, 70), maxlen - 1, maxlen, the rest
    random (half of them short).  with_x: about half of the reads get X at some of the bases 0, 15, 16, 31, 32, the last
    one, and a random one; one read is all X; the others (at least a third) have none.
    The first seed of a fixed sequence whose set covers every start phase (tests/test_loader_cases.py asserts that)."""
    for salt in range(64):
        reads = _ragged_reads(maxlen, with_x, salt)
        if start_phases(reads, 16) == set(range(16)) and (not with_x or start_phases(reads, 32, True) == set(range(32))):
            return reads
    raise AssertionError("no seed covers the start phases")


def _ragged_reads(maxlen, with_x, salt):
    rng = random.Random(7919 * maxlen + 2 * salt + (1 if with_x else 0))
    lens = list(range(0, min(maxlen, 70) + 1)) + [maxlen - 1, maxlen]
    while len(lens) < N_RAGGED:
        lens.append(rng.randint(0, min(maxlen, 70)) if rng.random() < 0.5 else rng.randint(0, maxlen))
    rng.shuffle(lens)
    reads = [rand_bases(rng, L) for L in lens]
    if with_x:
        all_x_done = False
        for i, r in enumerate(reads):
            L = len(r)
            if L == 0 or rng.random() < 0.45:
                continue
            if not all_x_done and L >= 33:
                reads[i] = b"X" * L
                all_x_done = True
                continue
            places = [p for p in X_PLACES + (L - 1,) if p < L and rng.random() < 0.4]
            places.append(rng.randrange(L))
            reads[i] = _put_x(rng, r, places)
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def fixed_reads(L, with_x):
    """N_FIXED reads of L bases.  with_x (the fixed-length loader with a mask): about half of the reads hold an X."""
    rng = random.Random(104729 * L + (1 if with_x else 0))
    reads = [rand_bases(rng, L) for _ in range(N_FIXED)]
    if with_x:
        for i, r in enumerate(reads):
            if rng.random() < 0.5:
                reads[i] = _put_x(rng, r, [rng.choice([0, L - 1, rng.randrange(L)])] + [p for p in X_PLACES if p < L and rng.random() < 0.2])
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def target_set(with_x):
    """Targets of the lengths TARGET_LENS in shuffled order, more of the same lengths until the database is longer than
    2 200 bases, and an empty target first, in the middle and last.  with_x: X at the first and the last base of three
    targets and at the database bases DB_X_BASES, the six bytes ODD_BYTES among them, each once."""
    rng = random.Random(31337)
    lens = list(TARGET_LENS)
    rng.shuffle(lens)
    while sum(lens) <= 2200 or sum(lens) % 16 == 0 or len({sum(lens[:i]) % 16 for i in range(len(lens))}) < 16:
        lens.append(rng.choice(TARGET_LENS))
    lens.insert(len(lens) // 2, 0)
    lens = [0] + lens + [0]
    targets = [bytearray(rand_bases(rng, L)) for L in lens]
    if with_x:
        starts = offsets_of(targets)
        for L in (257, 17, 1):  # (the first target of that length that none of DB_X_BASES falls into)
            g = next(g for g, n in enumerate(lens) if n == L and not any(starts[g] <= b < starts[g + 1] for b in DB_X_BASES))
            targets[g][0] = targets[g][-1] = ord("X")
        for base, odd in zip(DB_X_BASES, ODD_BYTES):
            g = int(np.searchsorted(starts, base, side="right")) - 1
            targets[g][base - int(starts[g])] = odd[0]
    return tuple(bytes(t) for t in targets)


def target_rests(targets):
    return [b"gene%d\t%d" % (g, len(t)) for g, t in enumerate(targets)]


def target_tuples(targets):
    """(0, g, 0, 0) for every target, and the first 257-base target at p = 1, 15, 16, 17 and 255 as well."""
    g257 = [len(t) for t in targets].index(257)
    return [(0, g, 0, 0) for g in range(len(targets))] + [(0, g257, p, 0) for p in (1, 15, 16, 17, 255)]


PREFIX_CUTS = tuple(c for k in range(1, 48) for c in (21 * k - 1, 21 * k, 21 * k + 1)) + (1000,)


@functools.lru_cache(maxsize=None)
def prefix_reads():
    """Prefixes of one 1000-base sequence (48 key words of 21 bases in the read prep's sort), cut on either side of
    every key-word boundary, each with near-twins that differ in their last base only, shuffled, with duplicates."""
    rng = random.Random(4242)
    seq = rand_bases(rng, 1000)
    reads = []
    for c in PREFIX_CUTS:
        p = seq[:c]
        reads.append(p)
        reads.append(p[:-1] + bytes([ACGT[(ACGT.index(p[-1]) + 1 + rng.randrange(3)) % 4]]))
        if c % 21 == 0:
            reads.append(p[:-1] + b"X")
    reads += [rng.choice(reads) for _ in range(60)]
    rng.shuffle(reads)
    return tuple(reads)


def with_duplicates(reads, seed):
    """`reads` plus a third as many repeats of some of them, shuffled (the input of musc_reads_sort_unique)."""
    rng = random.Random(seed)
    out = list(reads) + [rng.choice(reads) for _ in range(len(reads) // 3)]
    rng.shuffle(out)
    return out


def start_phases(seqs, modulus, only_x=False):
    """The residues mod `modulus` of the start offsets of the sequences (only_x: of those that hold an X)."""
    off = offsets_of(seqs)
    return {int(off[i]) % modulus for i, s in enumerate(seqs) if not only_x or has_x(s)}


def x_places(reads):
    """Which of the placements the X variant must show occur: {"first", "last", 15, 16, 31, 32, "all", "none"}."""
    seen = set()
    for r in reads:
        x = [i for i, c in enumerate(as_x(r)) if c == ord("X")]
        if not x:
            seen.add("none")
            continue
        if len(x) == len(r):
            seen.add("all")
        if x[0] == 0:
            seen.add("first")
        if x[-1] == len(r) - 1:
            seen.add("last")
        seen.update(p for p in (15, 16, 31, 32) if p in x)
    return seen
