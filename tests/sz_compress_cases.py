"""The compressing writer of framed snappy streams, in plain Python: a model of the rule of
muscato_amd/csrc/sz_compress_plan.hpp in its tile form, and the seeded cases.  It shares no code with the library; the
elements, the chunk builders and the strict decoder are those of tests/sz_cases.py.

The rule, per chunk of at most 65 536 bytes: positions are walked in tiles of 256; a position with four bytes left looks
its hash up in a table that holds the positions of all EARLIER tiles (the highest one per hash), a candidate counts only
with equal four bytes, the match extends to at most 64 bytes and to the chunk's end; after the look-ups the tile's
positions are inserted.  The second candidate of a position is the earliest position of its own tile with the same
12-bit key, if that lies in front of it; the longer match is taken, the near one when both are equal.  The parse is
greedy from the left.  A block of n - n // 8 bytes or more is dropped and the
chunk stored.

tests/test_sz_compress_cases.py holds the model to sz_cases.ref_decode and to the host writer without a GPU and asserts
the coverage listed in REQUIRED from the parse itself; tests/test_gpu_sz_compress.py runs the cases through the library."""
import functools
import random
import struct

import sz_cases

CHUNK = 65536
TILE = 256
HASH_BITS = 14
NEAR_BITS = 12
MAX_MATCH = 64


def hash4(v):
    return ((v * 0x1E35A7BD) & 0xFFFFFFFF) >> (32 - HASH_BITS)


class Parse:
    """One chunk under the rule.  copies = [(position, offset, length)], lits = [(position, length)] in stream order;
    elems = the elements as sz_cases makes them; rejected = positions whose table entry held other bytes (a hash
    collision); near = positions whose match is the near candidate's; both = {position: (far length, near length)}
    where both candidates match."""

    def __init__(self, data):
        n = len(data)
        assert 1 <= n <= CHUNK
        self.n = n
        self.copies, self.lits, self.elems, self.rejected, self.near, self.both = [], [], [], [], set(), {}
        table = {}
        words = [struct.unpack_from("<I", data, i)[0] for i in range(n - 3)]
        hashes = [hash4(v) for v in words]
        self.mlen = mlen = [0] * n
        moff = [0] * n

        def extend(j, i):
            room = min(MAX_MATCH, n - i)
            if data[j:j + room] == data[i:i + room]:
                return room
            m = 4
            while data[j + m] == data[i + m]:
                m += 1
            return m

        for t0 in range(0, n, TILE):
            t1 = min(t0 + TILE, n - 3)
            first = {}
            for i in range(t0, t1):
                first.setdefault(hashes[i] >> (HASH_BITS - NEAR_BITS), i)
            for i in range(t0, t1):
                j = table.get(hashes[i])
                if j is not None and words[j] != words[i]:
                    self.rejected.append(i)
                    j = None
                k = first[hashes[i] >> (HASH_BITS - NEAR_BITS)]
                if k < i and words[k] != words[i]:
                    self.rejected.append(i)
                mf = extend(j, i) if j is not None else 0
                mn = extend(k, i) if k < i and words[k] == words[i] else 0
                if mn >= 4 and mf >= 4:
                    self.both[i] = (mf, mn)
                if mn >= 4 and mn >= mf:
                    mlen[i], moff[i] = mn, i - k
                    self.near.add(i)
                elif mf >= 4:
                    mlen[i], moff[i] = mf, i - j
            for i in range(t0, t1):
                table[hashes[i]] = i  # (ascending: the highest position of the tile stays)
        p = start = 0
        while p < n:
            if mlen[p] >= 4:
                if start < p:
                    self.lits.append((start, p - start))
                    self.elems.append(sz_cases.lit(data[start:p]))
                self.copies.append((p, moff[p], mlen[p]))
                self.elems.append(sz_cases.copy(moff[p], mlen[p]))
                p += mlen[p]
                start = p
            else:
                p += 1
        if start < n:
            self.lits.append((start, n - start))
            self.elems.append(sz_cases.lit(data[start:]))
        self.element_bytes = sum(len(e[1]) for e in self.elems)
        self.block = sz_cases.varint(n) + sz_cases.encode_elements(self.elems)
        self.stored = len(self.block) >= n - n // 8

    def chunk(self, data):
        if self.stored:
            return sz_cases.plain_chunk(data)
        return sz_cases.chunk(0x00, sz_cases.stored_crc(data) + self.block)


@functools.lru_cache(maxsize=None)
def parses(plain):
    return tuple(Parse(plain[p:p + CHUNK]) for p in range(0, len(plain), CHUNK))


@functools.lru_cache(maxsize=None)
def model(plain):
    """The stream the writer makes of `plain`: the host's sz_encode_compressed and the device's musc_sz_compress."""
    return sz_cases.STREAM_ID + b"".join(P.chunk(plain[k * CHUNK:(k + 1) * CHUNK]) for k, P in enumerate(parses(plain)))


def bound(nbytes):
    return 10 + 8 * ((nbytes + CHUNK - 1) // CHUNK) + nbytes


# ---------------------------------------------------------------- building blocks

BINARY = bytes(b for b in range(256) if b not in b"\r\n")  # (no line ends: a FASTA record takes such a text as it is)


def uniq(rng, n, avoid=b""):
    """n random bytes in which no four bytes stand twice (and none of `avoid`'s): nothing in them matches by accident."""
    while True:
        d = bytes(rng.choice(BINARY) for _ in range(n))
        grams = [d[i:i + 4] for i in range(n - 3)]
        if len(set(grams)) == len(grams) and not any(g in avoid for g in grams if avoid):
            return d


def noise(seed, n):
    rng = random.Random(seed)
    return bytes(rng.choice(BINARY) for _ in range(n))


def run_tail(n, byte=b"Z"):
    """A run that makes a chunk worth keeping compressed, whatever stands in front of it."""
    return byte * n


def dna_lines(seed, nbytes, width=1000):
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < nbytes:
        out += bytes(rng.choice(b"ACGT") for _ in range(width)) + b"\n"
    return bytes(out[:nbytes])


def id_lines(seed, nbytes):
    rng = random.Random(seed)
    out, i = bytearray(), 0
    while len(out) < nbytes:
        out += b"%011d\tgene%d\t%d\n" % (i, i, rng.randint(200, 9000))
        i += 1
    return bytes(out[:nbytes])


def id_pair_lines(seed, nbytes):
    """The id text of a run with reverse complements: every name twice, the second time with _r.  The second line's best
    match is the first, some thirty bytes back and nearly always in its own tile: the text the near candidate is there
    for (without it the sequential model is ahead by 9 %)."""
    rng = random.Random(seed)
    out, i = bytearray(), 0
    while len(out) < nbytes:
        ln = rng.randint(200, 9000)
        out += b"%011d\tgene%d\t%d\n" % (2 * i, i, ln) + b"%011d\tgene%d_r\t%d\n" % (2 * i + 1, i, ln)
        i += 1
    return bytes(out[:nbytes])


def read_lines(seed, nbytes):
    rng = random.Random(seed)
    out, i = bytearray(), 0
    while len(out) < nbytes:
        out += bytes(rng.choice(b"ACGT") for _ in range(100)) + b"\tread%d/1\n" % i
        i += 1
    return bytes(out[:nbytes])


CORPORA = (("dna-lines", dna_lines), ("id-lines", id_lines), ("read-lines", read_lines), ("id-pair-lines", id_pair_lines))


@functools.lru_cache(maxsize=None)
def corpus(name):
    return dict(CORPORA)[name](11, CHUNK)


@functools.lru_cache(maxsize=None)
def colliding_keys():
    """Two different four-byte keys with one hash, by search."""
    seen = {}
    v = 0x41434754
    while True:
        h = hash4(v)
        if h in seen:
            return struct.pack("<I", seen[h]), struct.pack("<I", v)
        seen[h] = v
        v = (v * 1103515245 + 12345) & 0xFFFFFFFF


def threshold_text(rep):
    """A random part and a repeated part of `rep` bytes: the longer the repeat, the smaller the block against n - n / 8."""
    return uniq(random.Random(404), 4000) + run_tail(rep)


@functools.lru_cache(maxsize=None)
def threshold_rep():
    """The shortest repeated part with which the chunk is kept compressed (every shorter one is stored: asserted in
    tests/test_sz_compress_cases.py for the neighbour)."""
    lo, hi = 0, 4000  # stored at lo, compressed at hi
    assert Parse(threshold_text(hi)).stored is False and Parse(threshold_text(lo)).stored is True
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if Parse(threshold_text(mid)).stored:
            lo = mid
        else:
            hi = mid
    return hi


# ---------------------------------------------------------------- the cases

class Case:
    """name; plain; covers = what of REQUIRED it is there for (asserted from the parse by `shows`)."""

    def __init__(self, name, plain, covers=()):
        self.name, self.plain, self.covers = name, plain, set(covers)

    def __repr__(self):
        return self.name


REQUIRED = (
    ["len-%d" % n for n in (0, 1, 3, 4, 5, 255, 256, 257, 65535, 65536, 65537)] + ["nine-chunks", "ten-chunks"]
    + ["match-on-last-of-tile", "match-on-first-of-tile", "candidate-tile-before"]
    + ["near-candidate", "near-is-earliest", "near-on-tie", "far-longer"]
    + ["match-ends-at-n", "match-ends-at-n-1", "match-ends-at-n-2", "match-ends-at-n-3"]
    + ["copy1-off-2047-len-11", "copy2-off-2047-len-12", "copy2-off-2048-len-11", "copy2-off-2048-len-12", "off-65532"]
    + ["period-1", "period-2", "period-3", "capped-run", "lit-60", "lit-61", "lit-256", "lit-257", "lit-2-length-bytes"]
    + ["hash-collision", "stored-random", "threshold-stored", "threshold-compressed", "stored-and-compressed-chunks"]
    + ["dna-lines", "id-lines", "read-lines", "id-pair-lines"]
)

MOTIF = b"\x01muscato-motif-\x02\x03\x04\x05\x06\x07\x08\x09\x0a\x0b\x0c\x0d\x0e\x0f\x10\x11\x12\x13\x14\x15\x16\x17\x18\x19"  # no four bytes twice


@functools.lru_cache(maxsize=None)
def cases():
    rng = random.Random(2027)
    out = []
    text = dna_lines(5, 10 * CHUNK)

    for n in (0, 1, 3, 4, 5, 255, 256, 257):
        out.append(Case("len-%d" % n, (b"ACGTACGTTGCA" * 30)[:n], ["len-%d" % n]))
    for n in (65535, 65536, 65537):
        out.append(Case("len-%d" % n, text[:n], ["len-%d" % n]))
    out.append(Case("nine-chunks", text[:8 * CHUNK + 777], ["nine-chunks"]))
    out.append(Case("ten-chunks-ids", id_lines(3, 10 * CHUNK), ["ten-chunks"]))

    # ---- matches against the tile edges: planted in bytes where nothing else matches, a run behind them
    def planted(n, places, motif=MOTIF[:12], tail=3000, want=()):
        for _ in range(50):  # (another key of the same hash between the two places, or an equal byte behind them: draw again)
            d = bytearray(uniq(rng, n, avoid=MOTIF + b"ZZZZ"))
            for q in places:
                d[q:q + len(motif)] = motif
            d = bytes(d) + run_tail(tail)
            if set(want) <= shows(d):
                return d
        raise AssertionError("no text shows %s" % (want,))

    out.append(Case("match-on-last-of-tile", planted(1024, (10, 511), want=["match-on-last-of-tile"]), ["match-on-last-of-tile", "candidate-tile-before"]))
    out.append(Case("match-on-first-of-tile", planted(1024, (10, 512), want=["match-on-first-of-tile"]), ["match-on-first-of-tile"]))
    # ---- the near candidate: the tile's earliest position with the key; against the far one
    out.append(Case("near-candidate", planted(1024, (300, 340, 380), want=["near-candidate", "near-is-earliest"]),
                    ["near-candidate", "near-is-earliest"]))
    out.append(Case("near-on-tie", planted(1024, (10, 300, 340), want=["near-on-tie"]), ["near-on-tie", "candidate-tile-before"]))
    for _ in range(50):
        d = bytearray(planted(1024, (10, 340), motif=MOTIF[:20]))
        d[300:312] = MOTIF[:12]
        if "far-longer" in shows(bytes(d)):
            break
    out.append(Case("far-longer", bytes(d), ["far-longer"]))
    for d in (0, 1, 2, 3):
        body = planted(600, (100,), motif=MOTIF) + MOTIF[:20] + uniq(rng, 8, avoid=MOTIF)[:d]
        out.append(Case("match-ends-at-n-%d" % d, body, ["match-ends-at-n" + ("-%d" % d if d else "")]))
    for off in (2047, 2048):
        for ln in (11, 12):
            tag = "copy%d-off-%d-len-%d" % (1 if off < 2048 and ln <= 11 else 2, off, ln)
            out.append(Case("offset-%d-len-%d" % (off, ln), planted(2400, (100, 100 + off), motif=MOTIF[:ln], want=[tag]), [tag]))
    far = bytearray(uniq(rng, 1500, avoid=MOTIF + b"ZZZZ") + run_tail(CHUNK - 1500))
    far[0:4] = MOTIF[:4]
    far[CHUNK - 4:] = MOTIF[:4]
    out.append(Case("offset-65532", bytes(far), ["off-65532", "match-ends-at-n"]))

    # ---- overlapping copies and the cap
    out.append(Case("period-1", b"A" * 1000, ["period-1"]))
    out.append(Case("period-2", b"AC" * 500, ["period-2"]))
    out.append(Case("period-3", b"ACG" * 400 + b"T", ["period-3"]))
    out.append(Case("run-whole-chunk", b"G" * CHUNK, ["capped-run", "period-1", "len-65536"]))

    # ---- literal runs around the length bytes
    m8 = MOTIF[:8]
    d = bytearray(uniq(rng, 300, avoid=MOTIF + b"ZZZZ"))
    d[0:8] = m8
    for ln in (60, 61, 256, 257):
        d += m8 + uniq(rng, ln, avoid=MOTIF + b"ZZZZ")
    out.append(Case("literal-runs", bytes(d) + m8 + run_tail(3000), ["lit-60", "lit-61", "lit-256", "lit-257", "lit-2-length-bytes"]))

    # ---- two keys with one hash
    ka, kb = colliding_keys()
    d = bytearray(uniq(rng, 1024, avoid=MOTIF + b"ZZZZ"))
    d[10:14] = ka
    d[300:304] = kb
    out.append(Case("hash-collision", bytes(d) + run_tail(3000), ["hash-collision"]))

    # ---- stored chunks; both sides of n - n / 8
    out.append(Case("random-bytes", noise(9, CHUNK + 5000), ["stored-random"]))
    rep = threshold_rep()
    out.append(Case("threshold-stored", threshold_text(rep - 1), ["threshold-stored"]))
    out.append(Case("threshold-compressed", threshold_text(rep), ["threshold-compressed"]))
    out.append(Case("mixed-chunks", text[:CHUNK] + noise(10, CHUNK) + text[CHUNK:CHUNK + 999],
                    ["stored-and-compressed-chunks"]))

    # ---- the text corpora
    for name, _ in CORPORA:
        out.append(Case(name, corpus(name), [name, "len-65536"]))
    return tuple(out)


def shows(plain):
    """What of REQUIRED a text shows under the rule, read off its parse."""
    seen = set()
    n = len(plain)
    if n in (0, 1, 3, 4, 5, 255, 256, 257, 65535, 65536, 65537):
        seen.add("len-%d" % n)
    P = parses(plain)
    if len(P) == 9:
        seen.add("nine-chunks")
    if len(P) == 10:
        seen.add("ten-chunks")
    if any(p.stored for p in P) and any(not p.stored for p in P):
        seen.add("stored-and-compressed-chunks")
    for k, p in enumerate(P):
        data = plain[k * CHUNK:(k + 1) * CHUNK]
        if p.stored:
            if len(set(data)) > 200:
                seen.add("stored-random")
            continue  # (a dropped block shows nothing)
        for pos, off, ln in p.copies:
            if pos % TILE == TILE - 1:
                seen.add("match-on-last-of-tile")
            if pos % TILE == 0 and off > MAX_MATCH:
                seen.add("match-on-first-of-tile")
            if (pos - off) // TILE == pos // TILE - 1:
                seen.add("candidate-tile-before")
            for d in (0, 1, 2, 3):
                if pos + ln == p.n - d and ln < MAX_MATCH:
                    seen.add("match-ends-at-n" + ("-%d" % d if d else ""))
            if off in (2047, 2048) and ln in (11, 12):
                seen.add("copy%d-off-%d-len-%d" % (1 if off < 2048 and ln <= 11 else 2, off, ln))
            if off == 65532:
                seen.add("off-65532")
            if off in (1, 2, 3) and ln > off:
                seen.add("period-%d" % off)
        if len(p.copies) >= (CHUNK - TILE) // MAX_MATCH and len(set(data)) == 1:
            seen.add("capped-run")
        for pos, ln in p.lits:
            if ln in (60, 61, 256, 257):
                seen.add("lit-%d" % ln)
            if ln > 256:
                seen.add("lit-2-length-bytes")
        if any(data[i:i + 4] != data[i + 1:i + 5] for i in p.rejected):
            seen.add("hash-collision")
        for pos, off, ln in p.copies:
            if pos in p.near:
                assert (pos - off) // TILE == pos // TILE
                seen.add("near-candidate")
                if data.find(data[pos:pos + 4], pos - off + 1, pos + 3) != pos:
                    seen.add("near-is-earliest")  # (a nearer place with the same four bytes was not taken)
                if pos in p.both and p.both[pos][0] == p.both[pos][1]:
                    seen.add("near-on-tie")
            elif pos in p.both and p.both[pos][0] > p.both[pos][1]:
                seen.add("far-longer")
    if n == len(threshold_text(threshold_rep() - 1)) and P[0].stored and plain[:4000] == threshold_text(0):
        seen.add("threshold-stored")
    if n == len(threshold_text(threshold_rep())) and not P[0].stored and plain[:4000] == threshold_text(0):
        seen.add("threshold-compressed")
    for name, _ in CORPORA:
        if plain == corpus(name):
            seen.add(name)
    return seen
