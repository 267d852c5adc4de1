"""Framed snappy streams and gene-file texts for the device loader of the target database, in plain Python.

Three parts, none of which shares code with the library:
  - a stream builder with control of every element (literal length forms, copy widths, chunk headers, checksums), a small
    greedy compressor (a hash of four bytes) and a bitwise CRC-32C;
  - ref_decode, a strict decoder that states what the library must answer for a stream: the bytes, or the code (12 a
    refusal, 13 a bad stream), the number of the failing chunk and the message of host/sz.hpp;
  - the line cases and model_targets, a byte-by-byte model of (targets, n_odd, first_odd_target) under bufio's line rule
    and the cut at the first tab.
tests/test_sz_cases.py holds all of it to the oracle without a GPU and asserts the coverage listed in REQUIRED;
tests/test_gpu_db_text.py runs the cases through the library."""
import functools
import random

STREAM_ID = b"\xff\x06\x00\x00sNaPpY"
MAX_CHUNK = 65536


# ---------------------------------------------------------------- CRC-32C, bit by bit

def crc32c(data):
    c = 0xFFFFFFFF
    for b in data:
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
    return c ^ 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _crc_table():
    t = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        t.append(c)
    return tuple(t)


def crc32c_fast(data):
    """The same value by table (the long cases); test_sz_cases.py holds it to the bitwise one."""
    t = _crc_table()
    c = 0xFFFFFFFF
    for b in data:
        c = t[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def mask_crc(c):
    return ((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF


def stored_crc(plain):
    return mask_crc(crc32c_fast(plain)).to_bytes(4, "little")


# ---------------------------------------------------------------- elements of a block

def varint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def lit(data, nbytes=None):
    """A literal.  nbytes None: the shortest form; 0: the length in the tag (1..60 bytes); 1..4: that many length bytes."""
    n = len(data) - 1
    assert n >= 0
    if nbytes is None:
        nbytes = 0 if n < 60 else (n.bit_length() + 7) // 8
    if nbytes == 0:
        assert n < 60
        return ("lit", bytes([n << 2]) + data, data)
    assert n < 256 ** nbytes
    return ("lit", bytes([(59 + nbytes) << 2]) + n.to_bytes(nbytes, "little") + data, data)


def copy(off, length, width=None):
    """A copy element with a 1-, 2- or 4-byte offset (width None: the narrowest that takes it)."""
    if width is None:
        width = 1 if 4 <= length <= 11 and off < 2048 else 2 if off < 65536 else 4
    if width == 1:
        assert 4 <= length <= 11 and 0 <= off < 2048
        enc = bytes([1 | ((length - 4) << 2) | ((off >> 8) << 5), off & 0xFF])
    else:
        assert 1 <= length <= 64
        enc = bytes([(2 if width == 2 else 3) | ((length - 1) << 2)]) + off.to_bytes(width, "little")
    return ("copy", enc, (off, length))


def apply_elements(elems):
    """The bytes a list of elements stands for; None when a copy reaches before byte 0 (or has offset 0)."""
    out = bytearray()
    for kind, _, arg in elems:
        if kind == "lit":
            out += arg
        else:
            off, length = arg
            if off == 0 or off > len(out):
                return None
            for _ in range(length):
                out.append(out[-off])
    return bytes(out)


def encode_elements(elems):
    return b"".join(e[1] for e in elems)


# ---------------------------------------------------------------- chunks

def chunk(ctype, body):
    assert len(body) < 1 << 24
    return bytes([ctype]) + len(body).to_bytes(3, "little") + body


def plain_chunk(data, crc=None):
    return chunk(0x01, (stored_crc(data) if crc is None else crc) + data)


def comp_chunk(elems, declared=None, crc=None, plain=None):
    """A compressed chunk of these elements.  declared: the varint (default: what the elements make); crc: the stored
    word (default: that of the bytes the elements make)."""
    if plain is None:
        plain = apply_elements(elems)
    if declared is None:
        declared = len(plain)
    if crc is None:
        crc = stored_crc(plain if plain is not None else b"")
    return chunk(0x00, crc + varint(declared) + encode_elements(elems))


def compress(data):
    """Elements for `data` (at most one chunk's worth), greedily: a hash of the next four bytes finds the last place that
    began with them; a match of four or more becomes copies of at most 64 bytes, the rest literals."""
    assert len(data) <= MAX_CHUNK
    elems, table, i, start, n = [], {}, 0, 0, len(data)
    while i + 4 <= n:
        key = data[i:i + 4]
        j = table.get(key)
        table[key] = i
        if j is None:
            i += 1
            continue
        m = 4
        while i + m < n and data[j + m] == data[i + m]:  # (may run into the bytes being produced: an overlapping copy)
            m += 1
        if start < i:
            elems.append(lit(data[start:i]))
        off = i - j
        while m:
            take = min(m, 64)
            if m - take in (1, 2, 3):  # no copy shorter than four is left over
                take -= 4
            elems.append(copy(off, take))
            m -= take
            i += take
        start = i
    if start < n:
        elems.append(lit(data[start:]))
    return elems


def frame(data, compressed, chunk_bytes=MAX_CHUNK, ident=True):
    """`data` as a framed stream of chunks of chunk_bytes (the last one shorter), all compressed or all not."""
    out = [STREAM_ID] if ident else []
    for p in range(0, len(data), chunk_bytes):
        piece = data[p:p + chunk_bytes]
        out.append(comp_chunk(compress(piece), plain=piece) if compressed else plain_chunk(piece))
    return b"".join(out)


# ---------------------------------------------------------------- what a stream must decode to

class SzError(Exception):
    def __init__(self, code, index, text):
        Exception.__init__(self, "chunk %d: %s" % (index, text))
        self.code, self.index, self.text = code, index, text


def _block(buf, ulen, index):
    """The elements of a block behind its varint, each checked before it is applied (the first check that fails)."""
    out = bytearray()
    p, n = 0, len(buf)
    while p < n:
        tag = buf[p]
        p += 1
        t = tag & 3
        if t == 0:
            ln = tag >> 2
            if ln >= 60:
                nb = ln - 59
                if nb > n - p:
                    raise SzError(13, index, "snappy: truncated literal length")
                ln = int.from_bytes(buf[p:p + nb], "little")
                p += nb
            ln += 1
            if ln > n - p:
                raise SzError(13, index, "snappy: truncated literal")
            if ln > ulen - len(out):
                raise SzError(13, index, "snappy: length mismatch")
            out += buf[p:p + ln]
            p += ln
            continue
        nb = (1, 2, 4)[t - 1]
        if nb > n - p:
            raise SzError(13, index, "snappy: truncated copy")
        if t == 1:
            ln, off = ((tag >> 2) & 7) + 4, ((tag >> 5) << 8) | buf[p]
        else:
            ln, off = (tag >> 2) + 1, int.from_bytes(buf[p:p + nb], "little")
        p += nb
        if off == 0 or off > len(out):
            raise SzError(13, index, "snappy: bad copy offset")
        if ln > ulen - len(out):
            raise SzError(13, index, "snappy: length mismatch")
        for _ in range(ln):
            out.append(out[-off])
    if len(out) != ulen:
        raise SzError(13, index, "snappy: length mismatch")
    return bytes(out)


def ref_plan(raw):
    """The data chunks of a stream as (index, type, crc word, declared length, block bytes); the framing rules of sz.hpp's
    sz_decode with its messages, and the refusal (12) of a chunk that declares more than 65 536 bytes."""
    chunks, pos, index = [], 0, 0
    while pos < len(raw):
        if pos + 4 > len(raw):
            raise SzError(13, index, "sz: truncated chunk header")
        ctype, ln = raw[pos], int.from_bytes(raw[pos + 1:pos + 4], "little")
        pos += 4
        if pos + ln > len(raw):
            raise SzError(13, index, "sz: truncated chunk")
        body = raw[pos:pos + ln]
        pos += ln
        if ctype == 0xFF:
            if body != b"sNaPpY":
                raise SzError(13, index, "sz: bad stream identifier")
        elif ctype in (0, 1):
            if ln < 4:
                raise SzError(13, index, "sz: chunk too short")
            q, ulen = 4, ln - 4
            if ctype == 0:
                ulen, shift = 0, 0
                while True:
                    if q >= ln:
                        raise SzError(13, index, "snappy: truncated length")
                    b = body[q]
                    q += 1
                    ulen |= (b & 0x7F) << shift
                    if b < 0x80:
                        break
                    shift += 7
                    if shift > 35:
                        raise SzError(13, index, "snappy: bad length")
            if ulen > MAX_CHUNK:
                raise SzError(12, index, "sz: a chunk declares more than 65536 uncompressed bytes")
            chunks.append((index, ctype, int.from_bytes(body[:4], "little"), ulen, body[q:]))
        elif ctype < 0x80:
            raise SzError(13, index, "sz: reserved unskippable chunk")
        index += 1
    return chunks


def ref_decode(raw):
    """The decoded bytes, or SzError: framing errors and the refusal first (the whole stream is planned before a block is
    touched), then the first chunk in stream order whose block or checksum is bad."""
    out = []
    for index, ctype, crc, ulen, block in ref_plan(raw):
        plain = _block(block, ulen, index) if ctype == 0 else block
        if mask_crc(crc32c_fast(plain)) != crc:
            raise SzError(13, index, "sz: checksum mismatch")
        out.append(plain)
    return b"".join(out)


# ---------------------------------------------------------------- the stream cases

class Case:
    """name; stream; plain = the builder's own bytes (None: invalid); code / index / text = the answer for an invalid one;
    covers = what of REQUIRED it is there for; oracle_checks = oracle.snappy_framed_decode rejects it (it verifies no
    checksum, takes offset 0 and reads short slices at a truncation without complaint)."""

    def __init__(self, name, stream, plain, covers, code=0, index=None, text=None, oracle_checks=True):
        self.name, self.stream, self.plain, self.covers = name, stream, plain, set(covers)
        self.code, self.index, self.text, self.oracle_checks = code, index, text, oracle_checks

    def __repr__(self):
        return self.name


REQUIRED = (
    ["lit-inline-1", "lit-inline-60", "lit-1byte", "lit-2byte", "lit-3byte", "lit-4byte", "lit-4byte-nonminimal"]
    + ["copy-width-1", "copy-width-2", "copy-width-4"]
    + ["copy-off-1", "copy-off-2", "copy-off-3", "copy-off-len-1", "copy-off-len"]
    + ["copy-off-63-len-64", "copy-off-64-len-64", "copy-off-65-len-64", "copy-to-byte-0", "copy-before-byte-0"]
    + ["chunk-0-plain", "chunk-0-comp", "chunk-1-plain", "chunk-1-comp", "chunk-65536-plain", "chunk-65536-comp"]
    + ["chunk-65537-plain", "chunk-65537-comp", "skippable", "padding", "second-identifier"]
    + ["mid-truncated-header", "mid-truncated-chunk", "mid-bad-identifier", "mid-too-short", "mid-reserved",
       "mid-truncated-length", "mid-bad-length", "mid-truncated-literal-length", "mid-truncated-literal",
       "mid-truncated-copy", "mid-bad-offset"]
    + ["length-short", "length-long", "bitflip-data", "bitflip-crc", "acgt", "acgt-repeats"]
)

GOOD_A = b"ACGTTGCAAC" * 5 + b"\n"
GOOD_C = b"TTGACCA\tid\n" * 7


def _mid(name, middle, code, text, covers, oracle_checks=True, tail=None):
    """A bad chunk between two good ones (chunk numbers 1, 2, 3 behind the identifier)."""
    stream = STREAM_ID + plain_chunk(GOOD_A) + middle + (plain_chunk(GOOD_C) if tail is None else tail)
    return Case(name, stream, None, covers, code, 2, text, oracle_checks)


@functools.lru_cache(maxsize=None)
def stream_cases():
    rng = random.Random(2024)
    cases = []

    def good(name, chunks, plain, covers, ident=True):
        cases.append(Case(name, (STREAM_ID if ident else b"") + b"".join(chunks), plain, covers))

    def rnd(n):
        return bytes(rng.choice(b"ACGT") for _ in range(n))

    # ---- literals in each length form
    for n, nb, tag in ((1, 0, "lit-inline-1"), (2, 0, None), (59, 0, None), (60, 0, "lit-inline-60"), (61, 1, "lit-1byte"),
                       (256, 1, None), (257, 2, "lit-2byte"), (65536, 2, None), (300, 3, "lit-3byte"), (1000, 4, "lit-4byte"),
                       (5, 4, "lit-4byte-nonminimal"), (1, 1, None)):
        d = rnd(n)
        good("literal-%d-form-%d" % (n, nb), [comp_chunk([lit(d, nb)])], d, [tag] if tag else [])
    # ---- copies
    base = rnd(200)
    for off, ln, w, tags in ((1, 10, 1, ["copy-width-1", "copy-off-1"]), (2, 11, 1, ["copy-off-2"]), (3, 64, 2, ["copy-off-3", "copy-width-2"]),
                             (9, 10, 1, ["copy-off-len-1"]), (10, 10, 2, ["copy-off-len"]), (63, 64, 2, ["copy-off-len-1", "copy-off-63-len-64"]),
                             (64, 64, 2, ["copy-off-len", "copy-off-64-len-64"]), (65, 64, 4, ["copy-off-65-len-64", "copy-width-4"]),
                             (200, 64, 2, ["copy-to-byte-0"]), (200, 7, 1, ["copy-to-byte-0"]), (200, 33, 4, ["copy-to-byte-0"]),
                             (1, 64, 4, ["copy-off-1"]), (199, 4, 1, [])):
        el = [lit(base), copy(off, ln, w), lit(b"G")]
        good("copy-off-%d-len-%d-w%d" % (off, ln, w), [comp_chunk(el)], apply_elements(el), tags)
    el = [lit(base), copy(10, 64), copy(74, 64), copy(1, 64), copy(3, 5), lit(b"TT"), copy(2, 64)]  # copies of copies, no barrier-free luck
    good("copy-chain", [comp_chunk(el)], apply_elements(el), [])
    for w in (1, 2, 4):
        el = [lit(base), copy(201, 8, w)]
        cases.append(Case("copy-before-byte-0-w%d" % w, STREAM_ID + comp_chunk(el, declared=208, crc=b"\0\0\0\0"), None,
                          ["copy-before-byte-0"], 13, 1, "snappy: bad copy offset"))
    el = [lit(base), copy(0, 8, 2)]
    cases.append(Case("copy-offset-0", STREAM_ID + comp_chunk(el, declared=208, crc=stored_crc(base + base[:8])), None, [], 13, 1,
                      "snappy: bad copy offset", oracle_checks=False))
    # ---- chunk sizes
    big = rnd(65536)
    good("chunk-0-plain", [plain_chunk(GOOD_A), plain_chunk(b""), plain_chunk(GOOD_C)], GOOD_A + GOOD_C, ["chunk-0-plain"])
    good("chunk-0-comp", [plain_chunk(GOOD_A), comp_chunk([]), plain_chunk(GOOD_C)], GOOD_A + GOOD_C, ["chunk-0-comp"])
    good("only-empty-chunks", [plain_chunk(b""), comp_chunk([])], b"", [])
    good("no-chunk", [], b"", [])
    good("chunk-1-plain", [plain_chunk(b"A")], b"A", ["chunk-1-plain"])
    good("chunk-1-comp", [comp_chunk([lit(b"C")])], b"C", ["chunk-1-comp"])
    good("chunk-65536-plain", [plain_chunk(b"T"), plain_chunk(big), plain_chunk(b"GA")], b"T" + big + b"GA", ["chunk-65536-plain"])
    good("chunk-65536-comp", [plain_chunk(b"T"), comp_chunk(compress(big), plain=big), plain_chunk(b"GA")], b"T" + big + b"GA",
         ["chunk-65536-comp"])
    run = b"ACGTTGCA" * 8192
    good("chunk-65536-run", [comp_chunk(compress(run), plain=run)], run, [])
    big1 = big + b"A"
    cases.append(Case("chunk-65537-plain", STREAM_ID + plain_chunk(GOOD_A) + plain_chunk(big1), None, ["chunk-65537-plain"], 12, 2,
                      "sz: a chunk declares more than 65536 uncompressed bytes", oracle_checks=False))
    cases.append(Case("chunk-65537-comp", STREAM_ID + comp_chunk([lit(big1)]), None, ["chunk-65537-comp"], 12, 1,
                      "sz: a chunk declares more than 65536 uncompressed bytes", oracle_checks=False))
    # ---- chunks that carry no data
    good("skippable", [plain_chunk(GOOD_A), chunk(0x80, b"whatever"), chunk(0xFD, b""), plain_chunk(GOOD_C)], GOOD_A + GOOD_C, ["skippable"])
    good("padding", [chunk(0xFE, b"\0" * 37), plain_chunk(GOOD_A), chunk(0xFE, b"")], GOOD_A, ["padding"])
    good("second-identifier", [plain_chunk(GOOD_A), STREAM_ID, comp_chunk(compress(GOOD_C))], GOOD_A + GOOD_C, ["second-identifier"])
    good("no-identifier", [plain_chunk(GOOD_A)], GOOD_A, [], ident=False)
    # ---- every framing and block error, in the middle chunk of three
    ok = plain_chunk(b"GGCC\n")
    cases.append(Case("mid-truncated-header", STREAM_ID + plain_chunk(GOOD_A) + ok + b"\x01\x09", None, ["mid-truncated-header"], 13, 3,
                      "sz: truncated chunk header", oracle_checks=False))
    cases.append(_mid("mid-truncated-chunk", b"\x01" + (len(ok) + len(plain_chunk(GOOD_C))).to_bytes(3, "little") + ok[4:], 13,
                      "sz: truncated chunk", ["mid-truncated-chunk"], oracle_checks=False))
    cases.append(_mid("mid-bad-identifier", chunk(0xFF, b"sNaPpy"), 13, "sz: bad stream identifier", ["mid-bad-identifier"]))
    cases.append(_mid("mid-identifier-length", chunk(0xFF, b"sNaPpY\0"), 13, "sz: bad stream identifier", []))
    cases.append(_mid("mid-too-short", chunk(0x01, b"\0\0\0"), 13, "sz: chunk too short", ["mid-too-short"], oracle_checks=False))
    cases.append(_mid("mid-reserved-02", chunk(0x02, b"abcdefg"), 13, "sz: reserved unskippable chunk", ["mid-reserved"]))
    cases.append(_mid("mid-reserved-7f", chunk(0x7F, b""), 13, "sz: reserved unskippable chunk", ["mid-reserved"]))
    cases.append(_mid("mid-truncated-length-empty", chunk(0x00, b"\0\0\0\0"), 13, "snappy: truncated length", ["mid-truncated-length"]))
    cases.append(_mid("mid-truncated-length", chunk(0x00, b"\0\0\0\0\x85\x80"), 13, "snappy: truncated length", ["mid-truncated-length"]))
    cases.append(_mid("mid-bad-length", chunk(0x00, b"\0\0\0\0\x80\x80\x80\x80\x80\x80\x00"), 13, "snappy: bad length", ["mid-bad-length"],
                      oracle_checks=False))
    d = rnd(100)
    full = lit(d, 2)[1]
    cases.append(_mid("mid-truncated-literal-length", chunk(0x00, stored_crc(d) + varint(100) + full[:2]), 13,
                      "snappy: truncated literal length", ["mid-truncated-literal-length"]))
    cases.append(_mid("mid-truncated-literal", chunk(0x00, stored_crc(d) + varint(100) + full[:-1]), 13, "snappy: truncated literal",
                      ["mid-truncated-literal"]))
    for w in (1, 2, 4):
        enc = lit(d)[1] + copy(50, 8, w)[1][:-1]
        cases.append(_mid("mid-truncated-copy-w%d" % w, chunk(0x00, stored_crc(d + d[50:58]) + varint(108) + enc), 13, "snappy: truncated copy",
                          ["mid-truncated-copy"], oracle_checks=w != 4))
    cases.append(_mid("mid-bad-offset", comp_chunk([lit(d), copy(101, 8, 2)], declared=108, crc=b"\0\0\0\0"), 13, "snappy: bad copy offset",
                      ["mid-bad-offset"]))
    # ---- length mismatch, in both directions; one flipped bit
    el = [lit(d), copy(100, 20)]
    cases.append(_mid("length-short", comp_chunk(el, declared=121), 13, "snappy: length mismatch", ["length-short"]))
    cases.append(_mid("length-long-copy", comp_chunk(el, declared=119), 13, "snappy: length mismatch", ["length-long"]))
    cases.append(_mid("length-long-literal", comp_chunk([lit(d)], declared=99), 13, "snappy: length mismatch", ["length-long"]))
    flipped = bytearray(plain_chunk(d))
    flipped[8 + 41] ^= 0x10
    cases.append(_mid("bitflip-data-plain", bytes(flipped), 13, "sz: checksum mismatch", ["bitflip-data"], oracle_checks=False))
    flipped = bytearray(comp_chunk(el))
    flipped[-30] ^= 0x02  # a literal byte
    cases.append(_mid("bitflip-data-comp", bytes(flipped), 13, "sz: checksum mismatch", ["bitflip-data"], oracle_checks=False))
    flipped = bytearray(comp_chunk(el))
    flipped[4 + 3] ^= 0x80
    cases.append(_mid("bitflip-crc", bytes(flipped), 13, "sz: checksum mismatch", ["bitflip-crc"], oracle_checks=False))
    flipped = bytearray(plain_chunk(big))
    flipped[-1] ^= 0x01
    cases.append(_mid("bitflip-last-byte-of-65536", bytes(flipped), 13, "sz: checksum mismatch", ["bitflip-data"], oracle_checks=False))
    # ---- ACGT text through the compressor, with and without long repeats
    text = b"".join(rnd(rng.randint(1, 400)) + b"\n" for _ in range(700))
    good("acgt", [frame(text, True, ident=False)], text, ["acgt"])
    unit = [rnd(rng.randint(20, 3000)) for _ in range(6)]
    rep = b"".join(rng.choice(unit) + (b"\n" if rng.random() < 0.3 else b"") for _ in range(160)) + b"A" * 5000 + b"\n" + b"AC" * 4000
    good("acgt-repeats", [frame(rep, True, ident=False)], rep, ["acgt-repeats"])
    good("acgt-odd-chunks", [frame(text[:30011], True, chunk_bytes=997, ident=False)], text[:30011], [])
    good("acgt-odd-plain-chunks", [frame(text[:30011], False, chunk_bytes=1021, ident=False)], text[:30011], [])
    return tuple(cases)


# ---------------------------------------------------------------- gene-file texts

def model_targets(text):
    """(targets, n_odd, first_odd_target) of a gene file's text, one byte at a time.  A line ends at '\\n'; a last line
    without one is a line; nothing follows a final '\\n'.  The target is the line up to its first tab; a line without a
    tab loses one trailing '\\r'.  Odd = a target byte that is none of A C G T X; first_odd_target is 0 without one."""
    targets, cur, cut, n_odd, first = [], bytearray(), False, 0, None
    pending = False  # bytes since the last newline

    def close():
        nonlocal cur, cut
        if not cut and cur.endswith(b"\r"):
            del cur[-1]
        targets.append(bytes(cur))
        cur, cut = bytearray(), False

    for b in text:
        if b == 0x0A:
            close()
            pending = False
            continue
        pending = True
        if b == 0x09:
            cut = True
        if not cut:
            cur.append(b)
    if pending:
        close()
    for t, s in enumerate(targets):
        for b in s:
            if b not in b"ACGTX":
                n_odd += 1
                if first is None:
                    first = t
    return targets, n_odd, first or 0


def split_lines_cut(text):
    """The same targets as host/sz.hpp states them: split_lines (bufio.ScanLines), then the cut at the first tab."""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return [(ln[:-1] if ln.endswith(b"\r") else ln).split(b"\t")[0] for ln in lines]


LINE_REQUIRED = ["crlf", "cr-before-tab", "cr-cr", "unterminated", "final-newline", "empty-lines", "tab-first", "two-tabs",
                 "len-0", "len-1", "len-15", "len-16", "len-17", "len-31", "len-32", "len-33", "empty-run",
                 "nl-15", "nl-16", "nl-17", "nl-1023", "nl-1024", "nl-4095", "nl-4096", "nl-4097",
                 "long-target", "nl-first-of-chunk", "nl-last-of-chunk", "odd-N", "odd-lower", "odd-nul", "odd-high", "odd-cr", "x"]


@functools.lru_cache(maxsize=None)
def line_cases():
    """(name, text, covers).  The framed forms cut the text every 65 536 bytes (and, for the short ones, every 7)."""
    rng = random.Random(77)

    def rnd(n):
        return bytes(rng.choice(b"ACGT") for _ in range(n))

    cases = []
    cases.append(("rules", b"ACGT\r\nGG\tid\r\nTTA\r\tid\nCA\r\r\n\tid\nAC\tb\tc\n\n\r\nGATTACA", ["crlf", "cr-before-tab", "cr-cr", "unterminated",
                                                                                          "tab-first", "two-tabs", "empty-lines", "odd-cr"]))
    cases.append(("final-newline", b"ACGT\tgene0\t4\nTTGA\tgene1\t4\n", ["final-newline"]))
    cases.append(("one-newline", b"\n", ["len-0"]))
    cases.append(("one-base", b"G", ["len-1", "unterminated"]))
    cases.append(("one-cr", b"\r", []))
    lens = [0, 1, 15, 16, 17, 31, 32, 33, 0, 0, 0, 0, 5, 0, 0, 16, 16, 1, 1, 1, 33, 0]
    cases.append(("lengths", b"".join(rnd(n) + b"\n" for n in lens), ["len-%d" % n for n in (0, 1, 15, 16, 17, 31, 32, 33)] + ["empty-run"]))
    cases.append(("lengths-with-ids", b"".join(rnd(n) + b"\t%011d\tname%d\t%d\r\n" % (i, i, n) for i, n in enumerate(lens)), []))
    for at in (15, 16, 17, 1023, 1024, 4095, 4096, 4097):
        # newlines at `at` and around it, in a text with bases behind
        t = bytearray(rnd(at + 3000))
        for q in (at, at + 21, at + 22):
            t[q] = 0x0A
        cases.append(("newline-at-%d" % at, bytes(t), ["nl-%d" % at]))
    t = bytearray(rnd(3 * 65536 + 1000))  # one target over three chunk seams, then a newline as the first and as the last byte of a chunk
    t[3 * 65536 - 1] = 0x0A
    t[3 * 65536] = 0x0A
    t[3 * 65536 + 500] = 0x09
    cases.append(("long-target", bytes(t), ["long-target", "nl-first-of-chunk", "nl-last-of-chunk"]))
    odd = bytearray(rnd(300))
    for q, b in ((3, b"N"), (40, b"n"), (41, b"a"), (77, b"\0"), (130, b"\x80"), (131, b"\xff"), (200, b"X"), (201, b"X"), (250, b"-")):
        odd[q] = b[0]
    for q in (20, 60, 100, 160, 220, 280):
        odd[q] = 0x0A
    cases.append(("odd-bytes", bytes(odd) + b"\nACG\r\tid\n", ["odd-N", "odd-lower", "odd-nul", "odd-high", "x", "odd-cr"]))
    cases.append(("x-only", b"ACXGT\nXXXX\n" + rnd(40) + b"\n", ["x"]))
    cases.append(("odd-late", rnd(5000) + b"\n" + rnd(17) + b"\n\n" + rnd(7) + b"N" + rnd(9) + b"\tid\n", ["odd-N"]))
    return tuple(cases)


def line_covers(text):
    """What of LINE_REQUIRED a text shows (asserted in tests/test_sz_cases.py against what the case claims)."""
    targets, n_odd, _ = model_targets(text)
    seen = set()
    for n in (0, 1, 15, 16, 17, 31, 32, 33):
        if any(len(t) == n for t in targets):
            seen.add("len-%d" % n)
    for q in (15, 16, 17, 1023, 1024, 4095, 4096, 4097):
        if len(text) > q and text[q] == 0x0A:
            seen.add("nl-%d" % q)
    if any(len(t) > 65536 for t in targets):
        seen.add("long-target")
    if any(q % 65536 == 0 and text[q] == 0x0A for q in range(65536, len(text), 65536)):
        seen.add("nl-first-of-chunk")
    if any(text[q] == 0x0A for q in range(65535, len(text), 65536)):
        seen.add("nl-last-of-chunk")
    if any(not targets[i] and not targets[i + 1] and not targets[i + 2] for i in range(len(targets) - 2)):
        seen.add("empty-run")
    if b"\r\n" in text:
        seen.add("crlf")
    if b"\r\t" in text:
        seen.add("cr-before-tab")
        if any(t.endswith(b"\r") for t in targets):
            seen.add("odd-cr")
    if b"\r\r\n" in text:
        seen.add("cr-cr")
    if text and text[-1] != 0x0A:
        seen.add("unterminated")
    if text.endswith(b"\n") and len(text) > 1:
        seen.add("final-newline")
    if b"\n\n" in text:
        seen.add("empty-lines")
    if b"\n\t" in text or text.startswith(b"\t"):
        seen.add("tab-first")
    if any(ln.count(b"\t") >= 2 for ln in text.split(b"\n")):
        seen.add("two-tabs")
    joined = b"".join(targets)
    for tag, pred in (("odd-N", lambda b: b == ord("N")), ("odd-lower", lambda b: 97 <= b <= 122), ("odd-nul", lambda b: b == 0),
                      ("odd-high", lambda b: b >= 0x80), ("x", lambda b: b == ord("X"))):
        if any(pred(b) for b in joined):
            seen.add(tag)
    return seen
