"""tests/sz_cases.py held to the oracle, without a GPU: the builder's streams decode under
oracle.snappy_framed_decode to the builder's own bytes, the invalid ones are rejected by it wherever it checks (it
verifies no checksum, takes a copy offset of 0, and reads short slices at some truncations: those cases are held to the
module's strict decoder and its bitwise CRC-32C alone), and the list of cases covers what sz_cases.REQUIRED and
LINE_REQUIRED name.  The line model is held to split_lines + the cut at the first tab as host/sz.hpp states them, and,
for texts without '\\r' and tabs, to the oracle's own line rule (raw.split(b"\\n") less a final empty piece)."""
import os
import random

import pytest

from oracle import muscato_oracle as orc

import sz_cases as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prep_targets")


def test_crc32c_check_value():
    assert sc.crc32c(b"123456789") == 0xE3069283
    assert sc.crc32c(b"") == 0
    rng = random.Random(1)
    for n in (1, 2, 3, 4, 5, 63, 64, 65, 1000):
        d = bytes(rng.randrange(256) for _ in range(n))
        assert sc.crc32c_fast(d) == sc.crc32c(d)


def test_coverage_of_the_stream_cases():
    cases = sc.stream_cases()
    assert len({c.name for c in cases}) == len(cases)
    seen = set().union(*(c.covers for c in cases))
    assert seen >= set(sc.REQUIRED), sorted(set(sc.REQUIRED) - seen)
    assert seen <= set(sc.REQUIRED), sorted(seen - set(sc.REQUIRED))
    # what a tag claims is what the case holds
    by = {c.name: c for c in cases}
    assert len(by["chunk-65536-plain"].plain) == 65536 + 3 and len(by["chunk-65537-plain"].stream) > 65537
    assert sum(1 for c in cases if c.plain is None and c.index == 2 and c.stream.startswith(sc.STREAM_ID + sc.plain_chunk(sc.GOOD_A))) >= 20
    for name in ("acgt", "acgt-repeats"):
        c = by[name]
        assert len(c.stream) < len(c.plain) and len(c.plain) > 65536  # the compressor compresses, over more than one chunk
    assert len(by["acgt-repeats"].stream) * 4 < len(by["acgt-repeats"].plain)
    assert max(len(c.stream) for c in cases) < 400 * 1024


@pytest.mark.parametrize("case", [c for c in sc.stream_cases() if c.plain is not None], ids=repr)
def test_valid_streams_decode_to_the_builders_bytes(case):
    assert orc.snappy_framed_decode(case.stream) == case.plain
    assert sc.ref_decode(case.stream) == case.plain
    assert case.code == 0


@pytest.mark.parametrize("case", [c for c in sc.stream_cases() if c.plain is None], ids=repr)
def test_invalid_streams_are_rejected(case):
    with pytest.raises(sc.SzError) as ei:
        sc.ref_decode(case.stream)
    assert (ei.value.code, ei.value.index, ei.value.text) == (case.code, case.index, case.text)
    assert case.code in (12, 13)
    if case.oracle_checks:
        with pytest.raises((AssertionError, ValueError, IndexError)):
            orc.snappy_framed_decode(case.stream)
    elif case.text == "sz: checksum mismatch":
        # the oracle checks no CRC: it decodes, and the module's own bitwise CRC is what differs from the stored word
        index, ctype, crc, ulen, block = [k for k in sc.ref_plan(case.stream) if k[0] == case.index][0]
        plain = sc._block(block, ulen, index) if ctype == 0 else block
        assert sc.mask_crc(sc.crc32c(plain)) != crc
        orc.snappy_framed_decode(case.stream)


@pytest.mark.parametrize("n", ["06", "07"])
def test_the_go_streams_pass_the_crc(n):
    """The streams golang/snappy's writer made: every chunk's stored word is mask(crc32c) of its bytes, bit by bit."""
    with open(os.path.join(GOLDEN, n, "genes.txt.sz"), "rb") as f:
        raw = f.read()
    chunks = sc.ref_plan(raw)
    assert chunks
    out = []
    for index, ctype, crc, ulen, block in chunks:
        plain = sc._block(block, ulen, index) if ctype == 0 else block
        assert sc.mask_crc(sc.crc32c(plain)) == crc
        out.append(plain)
    assert b"".join(out) == orc.snappy_framed_decode(raw) == sc.ref_decode(raw)


def test_the_compressor_round_trips():
    rng = random.Random(9)
    for n in (0, 1, 3, 4, 5, 64, 65, 1000):
        for alphabet in (b"A", b"AC", b"ACGT", bytes(range(256))):
            d = bytes(rng.choice(alphabet) for _ in range(n))
            assert sc.apply_elements(sc.compress(d)) == d
            assert orc.snappy_framed_decode(sc.frame(d, True, chunk_bytes=97)) == d


# ---------------------------------------------------------------- lines

def test_coverage_of_the_line_cases():
    cases = sc.line_cases()
    seen = set()
    for name, text, covers in cases:
        shows = sc.line_covers(text)
        assert set(covers) <= shows, (name, sorted(set(covers) - shows))
        seen |= set(covers)
    assert seen >= set(sc.LINE_REQUIRED), sorted(set(sc.LINE_REQUIRED) - seen)
    assert max(len(text) for _, text, _ in cases) < 400 * 1024


@pytest.mark.parametrize("case", sc.line_cases(), ids=lambda c: c[0])
def test_line_model(case):
    _, text, _ = case
    targets, n_odd, first = sc.model_targets(text)
    assert targets == sc.split_lines_cut(text)
    if b"\r" not in text and b"\t" not in text:
        lines = text.split(b"\n")  # the oracle's line rule (read_fastq, prep_targets_fasta)
        if lines and lines[-1] == b"":
            lines.pop()
        assert targets == lines
    odd = [(t, b) for t, s in enumerate(targets) for b in s if b not in b"ACGTX"]
    assert n_odd == len(odd) and first == (odd[0][0] if odd else 0)


def test_line_model_on_random_texts():
    rng = random.Random(5)
    for _ in range(300):
        text = bytes(rng.choice(b"ACGTX\n\n\r\tN") for _ in range(rng.randint(0, 60)))
        if text:
            assert sc.model_targets(text)[0] == sc.split_lines_cut(text)
    assert sc.model_targets(b"") == ([], 0, 0)
