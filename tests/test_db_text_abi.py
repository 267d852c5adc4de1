"""musc_sz_decode and musc_db_load_text as the library exports them and as Python binds them (no GPU):
the symbols, the layout of musc_db_text_info against the header's declaration, the argtypes, and a refusal of the library
surfacing as MuscatoError."""
import ctypes

import pytest

from muscato_amd import DbTextInfo, Engine, MuscatoError, _lib, build as mbuild

import abi_header as ah

NEW = ("musc_sz_decode", "musc_db_load_text")


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
    fields = [(n, ah.SCALARS[ctype]) for n, ctype, _ in ah.struct_fields("musc_db_text_info")]
    assert fields == list(_lib.MuscDbTextInfo._fields_)
    assert [n for n, _ in fields] == ["n_targets", "n_bases", "n_odd", "first_odd_target", "reserved", "n_text_bytes", "n_chunks",
                                      "ms_decode", "ms_parse"]
    assert ctypes.sizeof(_lib.MuscDbTextInfo) == 3 * 8 + 2 * 4 + 2 * 8 + 2 * 4
    assert _lib.MuscDbTextInfo.n_text_bytes.offset == 32 and _lib.MuscDbTextInfo.ms_decode.offset == 48
    assert [f for f in DbTextInfo.__dataclass_fields__] == [n for n, _ in fields if n != "reserved"]


def test_argtypes(lib):
    vp, u64, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    assert lib.musc_sz_decode.argtypes == [vp, vp, u64, vp, u64, ci, ctypes.POINTER(u64)]
    assert lib.musc_db_load_text.argtypes == [vp, vp, u64, ci, ci, ctypes.POINTER(_lib.MuscDbTextInfo)]


def test_wrappers_raise_when_the_library_refuses(lib):
    """Both entry points refuse a NULL context with code 1; the wrappers turn that into MuscatoError."""
    n = ctypes.c_uint64(7)
    assert lib.musc_sz_decode(None, None, 0, None, 0, 0, ctypes.byref(n)) == 1
    assert lib.musc_db_load_text(None, None, 0, 0, -1, None) == 1
    e = Engine.__new__(Engine)  # no context: what a closed Engine holds
    e._lib, e._h = lib, None
    with pytest.raises(MuscatoError, match=r"musc_sz_decode failed \(1\)"):
        e.sz_decode(b"\xff\x06\x00\x00sNaPpY")
    with pytest.raises(MuscatoError, match=r"musc_db_load_text failed \(1\)"):
        e.load_db_text(b"ACGT\n")
