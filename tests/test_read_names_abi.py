"""The entry points of the read-name stage (musc_reads_names_order, musc_reads_prep_fastq_names, musc_reads_names_text,
DESIGN.md 23) as the library exports them and as Python binds them, without a GPU: the symbols, the layout of
musc_read_names against the header, the Engine methods, and a refusal of the library surfacing as MuscatoError."""
import ctypes

import pytest

from muscato_amd import Engine, MuscatoError, _lib, build as mbuild

import abi_header as ah

NAMES = ("musc_reads_names_order", "musc_reads_prep_fastq_names", "musc_reads_names_text")


@pytest.fixture(scope="module")
def lib():
    mbuild.build()
    return _lib.load()


def test_symbols(lib):
    for s in NAMES:
        assert s in _lib.SYMBOLS and hasattr(lib, s) and getattr(lib, s).argtypes is not None and getattr(lib, s).restype is ctypes.c_int
        assert ah.prototype(s)[0] == "int", s
    assert [len(getattr(lib, s).argtypes) for s in NAMES] == [11, 8, 8]
    assert lib.musc_abi_version() == 3  # additions only


def test_struct_layout_against_the_header():
    """A C program that includes the header prints the size and every field's offset; ctypes must agree."""
    fields = [k for k, _ in _lib.MuscReadNames._fields_]
    c = ah.c_layout(["musc_read_names"])["musc_read_names"]
    assert c["sizeof"] == ctypes.sizeof(_lib.MuscReadNames)
    assert {k: off for k, (off, _) in c["fields"].items()} == {k: getattr(_lib.MuscReadNames, k).offset for k in fields}
    assert [k for k, _, _ in ah.struct_fields("musc_read_names")] == fields


def test_wrappers_raise_when_the_library_refuses(lib):
    """Every entry point refuses a NULL context with code 1; the wrappers turn that into MuscatoError."""
    nb = ctypes.c_uint64(7)
    fp, info = _lib.MuscFastqPrep(), _lib.MuscReadNames()
    assert lib.musc_reads_names_order(None, None, 0, 0, None, None, 0, None, None, 0, None) == 1
    assert lib.musc_reads_prep_fastq_names(None, None, 0, 0, 0, 0, ctypes.byref(fp), ctypes.byref(info)) == 1
    assert lib.musc_reads_names_text(None, 0, 0, 1, None, 0, 0, ctypes.byref(nb)) == 1
    e = Engine.__new__(Engine)  # no context: what a closed Engine holds
    e._lib, e._h = lib, None
    for call in (lambda: e.names_order(b"@a\n", [0], [2], [0], [0, 1]), lambda: e.prep_fastq_names(b"", 1, 10), e.names_text,
                 lambda: e.names_text(1, 3, 4), lambda: e.names_text_into(0, 0, 1, None, 0, False)):
        with pytest.raises(MuscatoError, match=r"musc_reads_\w+ failed \(1\)"):
            call()
