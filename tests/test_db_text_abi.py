"""musc_sz_decode and musc_db_load_text as the library exports them and as Python binds them (no GPU):
the symbols, the layout of musc_db_text_info against the header's declaration, the argtypes, and a refusal of the library
surfacing as MuscatoError."""
import ctypes
import os
import re

import pytest

from muscato_amd import DbTextInfo, Engine, MuscatoError, _lib, build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("musc_sz_decode", "musc_db_load_text")
CTYPE = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float}


@pytest.fixture(scope="module")
def lib():
    mbuild.build()
    return _lib.load()


@pytest.fixture(scope="module")
def hdr():
    with open(os.path.join(ROOT, "include", "muscato_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def test_symbols(lib, hdr):
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(lib, s) and getattr(lib, s).restype is ctypes.c_int
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    assert lib.musc_abi_version() == 3  # additions only
    assert re.search(r"#define\s+MUSC_ABI_VERSION\s+3\b", hdr)


def test_struct_layout(hdr):
    m = re.search(r"typedef\s+struct\s+musc_db_text_info\s*\{(.*?)\}\s*musc_db_text_info\s*;", hdr, flags=re.S)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), CTYPE[ctype]) for n in names.split(",")]
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
