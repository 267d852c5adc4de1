"""The FASTQ cases and their model, without a GPU: the model against the oracle's read prep, what each
case covers, and the ABI of musc_reads_prep_fastq -- header, ctypes struct and the built library's exports."""
import ctypes
import os
import re

import pytest

from muscato_amd import _lib
from oracle import muscato_oracle as orc

import abi_header as ah
import fastq_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "muscato_amd", "csrc", "kernels_fastq.hpp")

BY_NAME = {c.name: c for c in fc.cases()}


def test_case_names_are_unique():
    assert len(BY_NAME) == len(fc.cases())


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_model_equals_oracle(name):
    """oracle.read_fastq -> prep_reads -> uniqify, on every case without a carriage return (the oracle keeps them)."""
    c = BY_NAME[name]
    if b"\r" in c.raw:
        assert name in ("crlf", "lone_cr")
        return
    cfg = orc.Config(Windows=[0], WindowWidth=4, MinReadLength=c.min_len, MaxReadLength=c.max_len)
    recs = orc.read_fastq(c.raw)
    m = fc.model(c.raw, c.min_len, c.max_len)
    assert m.n_records == len(recs)
    lines = orc.prep_reads(recs, cfg)
    assert m.n_reads == len(lines) == m.n_records - m.n_short
    assert [s + b"\t" + fc.short_name(n) for s, n in zip(m.seqs, m.names)] == lines
    exp = orc.uniqify(lines)
    assert fc.unique(m) == [(u.seq, u.count, u.names) for u in exp]
    for i in range(m.n_reads):  # the spans quote the text
        assert c.raw[m.name_off[i]:m.name_off[i] + m.name_len[i]] == m.names[i]
        assert c.raw[m.seq_off[i]:m.seq_off[i] + m.seq_len[i]].translate(fc.SUBX) == m.seqs[i]


def test_carriage_returns():
    """One trailing \\r of a line goes, as dropCR takes it; any other is data: an X in a sequence, itself in a name."""
    c = BY_NAME["crlf"]
    assert c.raw.count(b"\r\n") == c.raw.count(b"\n") == c.raw.count(b"\r") == 24
    m = fc.model(c.raw, c.min_len, c.max_len)
    plain = fc.model(c.raw.replace(b"\r", b""), c.min_len, c.max_len)
    assert m.n_reads == 6 and m.seqs == plain.seqs and m.names == plain.names and not any(b"X" in s for s in m.seqs)
    m = fc.model(BY_NAME["lone_cr"].raw, 1, 100)
    assert m.n_records == 3 and m.names == [b"@cr\rin name", b"@two\r"]
    assert m.seqs == [b"ACGTXACGTACGT", b"ACGTACGTACXX"] and m.n_short == 1  # "\r" alone: raw length 0


def test_strides_are_the_kernels():
    src = open(KERNELS).read()
    lane = int(re.search(r"#define FQ_LANE_BYTES (\d+)u", src).group(1))
    block = int(re.search(r"#define FQ_BLOCK (\d+)u", src).group(1))
    assert fc.STRIDES == (lane, lane * 64, lane * block)


def test_build_sees_the_new_header():
    from muscato_amd import build as mbuild
    assert KERNELS in mbuild.HEADERS  # (an edit of the kernels rebuilds the library)
    assert '#include "kernels_fastq.hpp"' in open(os.path.join(os.path.dirname(KERNELS), "muscato_hip.hip")).read()


def test_newlines_on_every_boundary():
    seen = set()
    for c in fc.cases():
        if c.mark and c.mark[0] == "newline":
            _, at, kind = c.mark
            assert c.raw[at] == 10 and c.raw[:at].count(b"\n") % 4 == kind
            seen.add((at, kind))
    assert seen == {(s - 1 + d, k) for s in fc.STRIDES for d in (0, 1) for k in range(4)}


def test_sizes():
    got = {c.mark[1]: c for c in fc.cases() if c.mark and c.mark[0] == "size"}
    assert sorted(got) == sorted({0, 1, 15, 16, 17} | {fc.TILE * k + d for k in (1, 2, 3) for d in (-1, 1)})
    for n, c in got.items():
        assert len(c.raw) == n
    assert fc.model(got[0].raw, 1, 60).n_records == 0 and fc.model(got[17].raw, 1, 60).n_records == 0
    assert fc.model(got[fc.TILE + 1].raw, 1, 60).n_records > 20


def test_line_shapes():
    c = BY_NAME["nl_run16"]
    at = c.mark[1]
    assert at % fc.LANE == 0 and c.raw[at:at + fc.LANE] == b"\n" * fc.LANE and c.raw[at - 1] == 10 and c.raw[at + fc.LANE] != 10
    m = fc.model(c.raw, c.min_len, c.max_len)
    assert b"" in m.names and b"" in m.seqs
    for name, mark in ((n, c.mark) for n, c in BY_NAME.items() if c.mark and c.mark[0] == "lines"):
        raw = BY_NAME[name].raw
        assert len(fc.scan_lines(raw)) == mark[1] and raw.endswith(b"\n") == mark[2]
        assert fc.model(raw, 1, 100).n_records == 5
    assert {BY_NAME["dangling_%d%s" % (k, o)].mark[1] for k in (1, 2, 3) for o in ("", "_open")} == {21, 22, 23}
    assert not BY_NAME["no_trailing_newline"].raw.endswith(b"\n")
    m = fc.model(BY_NAME["empty_lines"].raw, 0, 100)
    assert m.n_records == 4 and m.names == [b"", b"@e1", b"", b"@e3"] and m.seqs == [b"ACGT", b"", b"", b"GGCC"]
    m = fc.model(BY_NAME["at_lines"].raw, 1, 100)
    lines = BY_NAME["at_lines"].raw.split(b"\n")
    assert lines[2].startswith(b"@") and lines[3].startswith(b"@") and lines[7].startswith(b"@")
    assert m.names == [b"@a0", b"@a1"] and m.seqs == [b"ACGTACGTACGT", b"TTTTACGTACGT"]


def test_length_rules():
    c = BY_NAME["min_max"]
    assert c.mark[1] == (c.min_len - 1, c.min_len, c.max_len, c.max_len + 1)
    m = fc.model(c.raw, c.min_len, c.max_len)
    assert m.n_records == 5 and m.n_short == 1 and m.seq_len == [20, 50, 50, 35] and m.max_len == 50
    c = BY_NAME["long_read"]
    m = fc.model(c.raw, c.min_len, c.max_len)
    assert c.max_len == 65535 and m.max_len == 10000
    i = m.seq_len.index(10000)
    assert m.seq_off[i] // fc.TILE + 2 <= (m.seq_off[i] + 10000) // fc.TILE  # it spans whole workgroup tiles


def test_bytes_and_names():
    m = fc.model(BY_NAME["odd_bytes"].raw, 1, 200)
    assert m.seqs[0] == b"XXXXACGTXXXXXX" and m.seqs[1] == b"ACXGTXACXGT" and m.seqs[2] == b"ACGTXXACGTXXACGT"
    raw = BY_NAME["odd_bytes"].raw
    assert b"\x00" in raw and b"\xff" in raw and b"\x80" in raw and b"n" in raw and b"N" in raw
    assert set(m.seqs[3]) == set(b"ACGTX")
    c = BY_NAME["names"]
    m = fc.model(c.raw, c.min_len, c.max_len)
    assert sorted(m.name_len)[-2:] == [1000, 1001] and any(b"\t" in n for n in m.names) and any(n.startswith(b"@\t") for n in m.names)
    u = fc.unique(m)
    assert any(len(names) == 999 and names.endswith(b"...") for _, _, names in u)      # the joined names' rule
    assert any(b"@" + b"m" * 994 + b"..." in fc.short_name(n) for n in m.names)         # the single name's rule
    c = BY_NAME["dup_names"]
    u = fc.unique(fc.model(c.raw, c.min_len, c.max_len))
    assert [n for _, k, n in u if k == 6] == [b"@Zed;@a;@b;@b;@b!;@zeta"]                # names, not file order, decide


def test_big_text_needs_two_scan_levels():
    raw = BY_NAME["big"].raw
    assert 8 << 20 <= len(raw) <= 16 << 20
    assert len(raw) // fc.TILE > 2048  # (SCAN_TILE of kernels_common.hpp: 8 items x 256 lanes)
    m = fc.model(raw, 1, 100)
    assert m.n_reads == 40000 and 5000 < len(set(m.seqs)) <= 6000


# ---------------------------------------------------------------- the ABI

FIELDS = ("n_records", "n_short", "n_reads", "n_unique", "max_len", "reserved", "name_off", "seq_off", "name_len", "seq_len",
          "order", "ustart")


def test_struct_layout_equals_the_header():
    c = ah.c_layout(["musc_fastq_prep"])["musc_fastq_prep"]
    assert c["sizeof"] == ctypes.sizeof(_lib.MuscFastqPrep)
    assert [n for n, _ in _lib.MuscFastqPrep._fields_] == list(FIELDS) == [n for n, _, _ in ah.struct_fields("musc_fastq_prep")]
    assert [c["fields"][f][0] for f in FIELDS] == [getattr(_lib.MuscFastqPrep, f).offset for f in FIELDS]


def test_header_declares_and_library_exports():
    ret, params = ah.prototype("musc_reads_prep_fastq")
    assert ret == "int" and params[0].startswith("musc_ctx*")
    ret, params = ah.prototype("musc_fastq_prep_free")
    assert ret == "void" and params[0].startswith("musc_fastq_prep*")
    assert ah.constants()["MUSC_ABI_VERSION"] == 3
    assert {"musc_reads_prep_fastq", "musc_fastq_prep_free"} <= set(_lib.SYMBOLS)
    lib = _lib.load()  # raises when a symbol of SYMBOLS is not exported
    assert hasattr(lib, "musc_reads_prep_fastq") and hasattr(lib, "musc_fastq_prep_free")
