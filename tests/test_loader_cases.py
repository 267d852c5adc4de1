"""The inputs of the loader readback tests (tests/loader_cases.py), checked without a GPU: every set still covers the
phases, strides and X placements it exists for, the expected text is what it should be, and muscato_amd.api.pack_2bit
-- which packs what Engine.load_reads_packed / load_targets_packed upload -- agrees with the reference packer."""
import random

import numpy as np
import pytest

from muscato_amd.api import concat, pack_2bit

import loader_cases as lc


def test_record_strides_reached():
    assert tuple(lc.record_words(m) for m in lc.RAGGED_MAXLENS) == lc.RAGGED_STRIDES
    # each maxlen is the last length of its stride or the first of the next
    for m in (48, 112, 176, 240):
        assert lc.record_words(m) + 4 == lc.record_words(m + 1) and (m + 1) in lc.RAGGED_MAXLENS
    assert lc.record_words(0) == lc.record_words(1) == 4 and lc.record_words(65535) == 4100


@pytest.mark.parametrize("with_x", [False, True])
@pytest.mark.parametrize("maxlen", lc.RAGGED_MAXLENS)
def test_ragged_sets_cover_their_phases(maxlen, with_x):
    reads = lc.ragged_reads(maxlen, with_x)
    lens = [len(r) for r in reads]
    assert len(reads) == lc.N_RAGGED and max(lens) == maxlen
    assert set(range(0, min(maxlen, 70) + 1)) | {maxlen - 1, maxlen} <= set(lens)
    assert lc.start_phases(reads, 16) == set(range(16))  # the phases of a 2-bit word
    assert all(set(r) <= set(b"ACGTX") for r in reads)
    if with_x:
        assert lc.start_phases(reads, 32, only_x=True) == set(range(32))  # the phases of a mask word
        assert lc.x_places(reads) == {"first", "last", 15, 16, 31, 32, "all", "none"}
        assert 3 * sum(1 for r in reads if not lc.has_x(r)) >= len(reads)
        assert sum(1 for r in reads if r and set(r) == {ord("X")} and len(r) >= 33) >= 1
    else:
        assert not any(lc.has_x(r) for r in reads)
    # the same bases with and without X, so that a difference between the variants is the X alone
    plain = lc.ragged_reads(maxlen, False)
    assert [len(r) for r in plain] != sorted(len(r) for r in plain)  # shuffled
    assert reads is lc.ragged_reads(maxlen, with_x)  # made once, shared


@pytest.mark.parametrize("L", lc.FIXED_LENS)
def test_fixed_sets(L):
    reads = lc.fixed_reads(L, False)
    assert len(reads) == lc.N_FIXED == 1000 and lc.N_FIXED % 64 and all(len(r) == L for r in reads)
    assert not any(lc.has_x(r) for r in reads)
    xr = lc.fixed_reads(L, True)
    assert all(len(r) == L for r in xr)
    nx = sum(1 for r in xr if lc.has_x(r))
    assert 3 * (len(xr) - nx) >= len(xr) and nx >= 100
    assert {"first", "last", "none"} <= lc.x_places(xr)
    # the bit phases a read's first base can have in the 64-bit extraction of the fixed-length packer
    phases = {(2 * r * L) % 32 for r in range(lc.N_FIXED)}
    assert len(phases) == (16 if L % 2 else 16 // np.gcd(L, 16))


def test_fixed_lengths_reach_every_bit_phase():
    assert any(L % 2 for L in lc.FIXED_LENS) and any(L % 2 == 0 and L % 16 for L in lc.FIXED_LENS)
    assert {lc.record_words(L) for L in lc.FIXED_LENS} == {4, 8, 12, 20}
    assert {L % 16 for L in lc.FIXED_LENS} >= {0, 1, 15}


@pytest.mark.parametrize("with_x", [False, True])
def test_target_sets(with_x):
    targets = lc.target_set(with_x)
    lens = [len(t) for t in targets]
    assert set(lens) == set(lc.TARGET_LENS) | {0}
    assert lens[0] == 0 and lens[-1] == 0 and lens.count(0) == 3 and 0 in lens[1:-1]
    total = sum(lens)
    assert total % 16 != 0 and total > 2200 > max(lc.DB_X_BASES)
    assert lc.start_phases(targets, 16) == set(range(16))
    assert lens == [len(t) for t in lc.target_set(not with_x)]
    db = b"".join(targets)
    if with_x:
        assert all(db[b:b + 1] not in (b"A", b"C", b"G", b"T") for b in lc.DB_X_BASES)
        assert all(db.count(odd) == 1 for odd in lc.ODD_BYTES)
        assert sum(1 for t in targets if t and t[:1] == b"X" and t[-1:] == b"X") >= 3
        assert b"X" not in lc.as_x(db).replace(b"X", b"") and lc.as_x(db).count(b"X") >= 6 + 5
    else:
        assert set(db) <= set(b"ACGT")
    hits = lc.target_tuples(targets)
    assert len(hits) == len(targets) + 5 and len(targets[hits[-1][1]]) == 257


def test_prefix_reads():
    reads = lc.prefix_reads()
    uniq = sorted(set(reads))
    lens = {len(r) for r in uniq}
    assert lens == set(lc.PREFIX_CUTS) and {20, 21, 22, 41, 42, 43, 987, 988, 1000} <= lens
    assert (1000 + 20) // 21 == 48 and len(reads) > len(uniq)
    longest = max(uniq, key=len)
    stems = [r for r in uniq if longest.startswith(r)]
    assert len(stems) == len(lc.PREFIX_CUTS) and stems == sorted(stems, key=len)  # a prefix sorts before its extensions
    twins = [r for r in uniq if not longest.startswith(r) and longest.startswith(r[:-1])]
    assert len(twins) >= len(lc.PREFIX_CUTS)
    assert any(r.endswith(b"X") for r in twins)


def test_expected_lines():
    reads = [b"ACGTX", b"", b"ACnT"]
    targets = [b"ACGTACGT", b"", b"GN-\x00\xffT"]
    rests = [b"a\t8", b"b\t0", b"c\t6"]
    hits = [(0, 0, 0, 0), (0, 0, 5, 2), (1, 1, 0, 0), (2, 2, 1, 65535), (0, 2, 6, 0), (1, 0, 3, 1)]
    assert lc.expected_lines(reads, targets, rests, hits) == [
        b"ACGTX\tACGTA\t0\t0\ta\t8\n", b"ACGTX\tCGT\t5\t2\ta\t8\n", b"\t\t0\t0\tb\t0\n", b"ACXT\tXXXX\t1\t65535\tc\t6\n",
        b"ACGTX\t\t6\t0\tc\t6\n", b"\t\t3\t1\ta\t8\n"]


def test_ref_pack_by_hand():
    b2, bm, nx = lc.ref_pack(b"ACGTTXGCA")
    assert nx == 1 and b2[:3].tolist() == [0b11100100, 0b01100011, 0b00] and bm[:2].tolist() == [0b00100000, 0]
    assert len(b2) == 3 + 16 and len(bm) == 2 + 16 and not b2[3:].any() and not bm[2:].any()
    g2, gm, _ = lc.ref_pack(b"ACGTTXGCA", random.Random(1))
    assert (gm == bm).all() and (g2[1] >> 2) & 3 != 0  # a non-zero code under the mask bit, nothing else changed
    assert g2[0] == b2[0] and g2[1] & 0b11110011 == b2[1] and g2[2] == b2[2]


def _pack_2bit_inputs():
    for m in lc.RAGGED_MAXLENS:
        for x in (False, True):
            yield "ragged-%d-%s" % (m, x), lc.ragged_reads(m, x)
    for L in lc.FIXED_LENS:
        yield "fixed-%d" % L, lc.fixed_reads(L, False)
    for L in (1, 37, 250):
        yield "fixedx-%d" % L, lc.fixed_reads(L, True)
    for x in (False, True):
        yield "targets-%s" % x, lc.target_set(x)


def test_pack_2bit_against_the_reference_packer():
    for name, seqs in _pack_2bit_inputs():
        buf, off = concat(seqs)
        n = int(off[-1])
        assert (off == lc.offsets_of(seqs)).all()
        packed, mask = pack_2bit(buf, n)
        b2, bm, nx = lc.ref_pack(b"".join(seqs))
        assert len(packed) == (n + 3) // 4 and (packed == b2[:len(packed)]).all(), name
        if nx:
            assert mask is not None and len(mask) == (n + 7) // 8 and (mask == bm[:len(mask)]).all(), name
        else:
            assert mask is None and not bm.any(), name
