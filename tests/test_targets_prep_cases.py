"""The target-preparation cases and their model (tests/targets_prep_cases.py) without a GPU: the model against the
oracle's prep_targets_text / prep_targets_fasta on every case and on seeded random texts, against the reference's
plain-text fixtures, the coverage the GPU tests rely on, and the new entry points as the library exports them and as
Python binds them."""
import ctypes
import os
import subprocess

import pytest

from muscato_amd import Engine, MuscatoError, TargetsPrepInfo, _lib, build as mbuild
from oracle import muscato_oracle as orc

import abi_header as ah
import sz_cases as sc
import targets_prep_cases as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "muscato_amd", "bin")
NEW = ("musc_targets_prep", "musc_targets_prep_text", "musc_targets_prep_load", "musc_targets_prep_free", "musc_sz_frame")


def check_against_oracle(text, fasta, rev):
    m = tp.model(text, fasta, rev)
    fed = tp.oracle_text(text)  # the oracle has no \r rule: it gets the text after bufio's
    if m.refused is not None:
        assert fasta and tp.lines_of(text)[m.refused] == b"" and b"" not in tp.lines_of(text)[:m.refused]
        with pytest.raises(IndexError):
            orc.prep_targets_fasta(fed, rev)
        return m
    seqs, ids = (orc.prep_targets_fasta if fasta else orc.prep_targets_text)(fed, rev)
    assert m.seqs == seqs and m.ids == ids
    return m


@pytest.mark.parametrize("rev", [False, True])
def test_model_equals_the_oracle_on_every_case(rev):
    for c in tp.all_cases():
        check_against_oracle(c.text, c.fasta, rev)


def test_model_equals_the_oracle_on_random_texts():
    refused = 0
    for i, text in enumerate(tp.random_texts(99, 6000)):
        for fasta in (False, True):
            refused += check_against_oracle(text, fasta, bool(i & 1)).refused is not None
    assert 500 < refused < 5500


@pytest.mark.parametrize("case,fname,rev", [("00", "genes.fasta", False), ("01", "genes.fasta", True), ("02", "genes.txt", False),
                                            ("03", "genes.txt", True)])
def test_model_equals_the_reference_fixtures(golden_dir, case, fname, rev):
    d = os.path.join(golden_dir, "prep_targets", case)
    with open(os.path.join(d, fname), "rb") as f:
        m = tp.model(f.read(), fname.endswith("fasta"), rev)
    seqs, ids = tp.texts_of(m)
    with open(os.path.join(d, "expected_sequences.txt"), "rb") as f:
        assert seqs == f.read()
    with open(os.path.join(d, "expected_ids.txt"), "rb") as f:
        assert ids == f.read()


def test_every_tag_is_covered():
    seen = set()
    for c in tp.all_cases():
        assert c.covers <= set(tp.REQUIRED), c.name
        seen |= c.covers
    assert set(tp.REQUIRED) - seen == set()


def test_cases_show_what_their_tags_say():
    by = {c.name: c for c in tp.all_cases()}
    for B in tp.BOUNDARIES:
        for kind, ch in (("nl", b"\n"), ("tab", b"\t"), ("gt", b">")):
            for fmt in ("fa", "tx"):
                t = by["%s_%s_%d_last" % (fmt, kind, B)].text
                assert t[B - 1:B] == ch and t[B:B + 1] != ch
                t = by["%s_%s_%d_first" % (fmt, kind, B)].text
                assert t[B:B + 1] == ch and t[B - 1:B] != ch
                t = by["%s_%s_%d_straddle" % (fmt, kind, B)].text
                assert t[B - 1:B + 1] == ch * 2
    assert by["fa_nl8"].text[16:32].count(b"\n") == 8 and by["tx_nl8"].text[16:32].count(b"\n") == 8
    assert by["fa_rec3"].text[16:31] == b">a\nA\n" * 3
    m = tp.model(by["fa_long_line"].text, True, False)
    assert len(m.seqs[0]) == 3 * 4096 + 5 and m.n_subx > 0
    m = tp.model(by["fa_300_lines"].text, True, True)
    assert by["fa_300_lines"].text.count(b"\n") == 2 + 1 + 300 + 2 and len(m.seqs) == 6
    m = tp.model(by["fa_3_tiles"].text, True, False)
    assert len(m.seqs[1]) == 9000
    assert len(tp.lines_of(by["fa_hdr_5000"].text)[2]) == 5000 and b"\t" in tp.lines_of(by["fa_hdr_5000"].text)[2]
    # the last record keeps its bytes, its complement holds NUL; the same bytes earlier are substituted
    m = tp.model(by["fa_last_raw"].text, True, True)
    assert b"\x00" in m.seqs[-2] and b"\xff" in m.seqs[-2] and b"n" not in m.seqs[0] and b"\x00" in m.seqs[-1] and b"\x00" not in m.seqs[1]
    assert [tp.model(by[n].text, True, False).refused for n in ("fa_empty_first", "fa_empty_mid", "fa_empty_last", "fa_lone_cr")] == [0, 3, 4, 2]
    assert tp.model(by["tx_lone_cr"].text, False, False).stop_line == 1
    m = tp.model(by["tx_stops_3_tiles"].text, False, False)
    stops = [k for k, l in enumerate(tp.lines_of(by["tx_stops_3_tiles"].text)) if not l or l.count(b"\t") != 1]
    pos = [sum(len(l) + 1 for l in tp.lines_of(by["tx_stops_3_tiles"].text)[:k]) // 4096 for k in stops]
    assert m.stop_line == stops[0] == 100 and len(set(pos)) == 3 and len(m.seqs) == 100
    assert tp.model(by["tx_stop0"].text, False, True).stop_line == 0
    assert tp.model(by["fa_nobases"].text, True, False).n_dropped == 4
    for n in tp.COUNTS:
        assert len(tp.model(by["fa_nrec_%d" % n].text, True, False).seqs) == n
        if n:
            m = tp.model(by["tx_nrec_%d" % n].text, False, True)
            assert len(m.seqs) == 2 * n and m.stop_line == tp.NO_STOP
    for name in ("fa_lens", "fa_lens_big", "tx_lens", "tx_lens_big"):
        c = by[name]
        assert {"len:%d:%s" % (len(s), "fasta" if c.fasta else "text") for s in tp.model(c.text, c.fasta, False).seqs} >= c.covers


# ---------------------------------------------------------------- the entry points (no GPU)

@pytest.fixture(scope="module")
def lib():
    mbuild.build()
    return _lib.load()


def test_symbols(lib):
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(lib, s) and getattr(lib, s).restype is ctypes.c_int
        assert ah.prototype(s)[0] == "int", s
    assert lib.musc_abi_version() == 3  # additions only
    assert ah.constants()["MUSC_ABI_VERSION"] == 3


def test_struct_layout():
    fields = [(n, ah.SCALARS[ctype]) for n, ctype, _ in ah.struct_fields("musc_targets_prep_info")]
    assert fields == list(_lib.MuscTargetsPrepInfo._fields_)
    assert [n for n, _ in fields] == ["n_lines", "n_records", "n_targets", "n_dropped", "stop_line", "n_subx", "n_seq_bytes", "n_id_bytes",
                                      "ms", "reserved"]
    assert ctypes.sizeof(_lib.MuscTargetsPrepInfo) == 8 * 8 + 2 * 4
    assert _lib.MuscTargetsPrepInfo.n_id_bytes.offset == 56 and _lib.MuscTargetsPrepInfo.ms.offset == 64
    assert [f for f in TargetsPrepInfo.__dataclass_fields__] == [n for n, _ in fields if n != "reserved"]


def test_argtypes(lib):
    vp, u64, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    assert lib.musc_targets_prep.argtypes == [vp, vp, u64, ci, ci, ci, ctypes.POINTER(_lib.MuscTargetsPrepInfo)]
    assert lib.musc_targets_prep_text.argtypes == [vp, ci, u64, u64, vp, ci]
    assert lib.musc_targets_prep_load.argtypes == [vp, ctypes.POINTER(_lib.MuscDbTextInfo)]
    assert lib.musc_targets_prep_free.argtypes == [vp]
    assert lib.musc_sz_frame.argtypes == [vp, vp, u64, ci, vp, u64, ci, ctypes.POINTER(u64)]
    # and against the prototypes: as many parameters, pointers as pointers, 64-bit integers as 64-bit
    for name in NEW:
        params = ah.prototype(name)[1]
        at = getattr(lib, name).argtypes
        assert len(at) == len(params), name
        for decl, ct in zip(params, at):
            assert ("*" in decl) == (ct is vp or hasattr(ct, "contents")), (name, decl)
            if "*" not in decl:
                assert ctypes.sizeof(ct) == (8 if "uint64_t" in decl else 4), (name, decl)


def test_wrappers_raise_when_the_library_refuses(lib):
    """Every new entry point refuses a NULL context with code 1; the wrappers turn that into MuscatoError."""
    n = ctypes.c_uint64(7)
    assert lib.musc_targets_prep(None, None, 0, 0, 0, 0, None) == 1
    assert lib.musc_targets_prep_text(None, 0, 0, 0, None, 0) == 1
    assert lib.musc_targets_prep_load(None, None) == 1
    assert lib.musc_targets_prep_free(None) == 1
    assert lib.musc_sz_frame(None, None, 0, 0, None, 0, 0, ctypes.byref(n)) == 1
    e = Engine.__new__(Engine)  # no context: what a closed Engine holds
    e._lib, e._h = lib, None
    for call, what in ((lambda: e.prep_targets(b">a\nACGT\n", True, False), "musc_targets_prep"),
                       (lambda: e.prepared_text(0, 0, 4), "musc_targets_prep_text"),
                       (lambda: e.load_db_prepared(), "musc_targets_prep_load"),
                       (lambda: e.free_prepared(), "musc_targets_prep_free"),
                       (lambda: e.sz_frame(b"ACGT"), "musc_sz_frame")):
        with pytest.raises(MuscatoError, match=r"%s failed \(1\)" % what):
            call()


@pytest.mark.parametrize("n", [0, 1, 65535, 65536, 65537, 131072, 131073])
def test_frame_size(n):
    """What musc_sz_frame sizes, 10 + 8 * ceil(n / 65536) + n, is the length of the stream of uncompressed chunks."""
    data = bytes(i * 7 & 0xFF for i in range(n))
    stream = sc.frame(data, False)
    assert len(stream) == 10 + 8 * ((n + 65535) // 65536) + n
    assert orc.snappy_framed_decode(stream) == data


def test_frame_equals_the_host_writer(tmp_path):
    """sc.frame(data, False), the GPU tests' reference for musc_sz_frame, is byte for byte what sz_encode writes: through
    the tool (on the host, its default) on a text of three chunks."""
    mbuild.build()
    c = next(c for c in tp.all_cases() if c.name == "tx_lens_big")
    (tmp_path / "genes.txt").write_bytes(c.text)
    env = {k: v for k, v in os.environ.items() if k != "MUSC_PREP_TARGETS"}
    r = subprocess.run([os.path.join(BIN, "muscato_prep_targets"), "-rev", "genes.txt"], cwd=tmp_path, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr
    seqs, ids = tp.texts_of(tp.model(c.text, False, True))
    assert len(seqs) > 2 * 65536
    assert (tmp_path / "musc_genes.txt.sz").read_bytes() == sc.frame(seqs, False)
    assert (tmp_path / "musc_ids_genes.txt.sz").read_bytes() == sc.frame(ids, False)
