"""The side-output entry points (musc_side_*) as the library exports them and as Python binds them (no
GPU): the symbols, the values of the `which` enum, and a refusal of the library surfacing as MuscatoError."""
import ctypes

import pytest

from muscato_amd import Engine, MuscatoError, _lib, build as mbuild

import abi_header as ah

SIDE = ("musc_side_prepare", "musc_side_text", "musc_side_last_ms")


@pytest.fixture(scope="module")
def lib():
    mbuild.build()
    return _lib.load()


def test_symbols_and_enum(lib):
    for s in SIDE:
        assert s in _lib.SYMBOLS and hasattr(lib, s) and getattr(lib, s).argtypes is not None and getattr(lib, s).restype is ctypes.c_int
        assert ah.prototype(s)[0] == "int", s
    c = ah.constants()
    assert [c["MUSC_SIDE_NONMATCH"], c["MUSC_SIDE_GENESTATS"], c["MUSC_SIDE_READSTATS"]] == [0, 1, 2] \
        == [_lib.SIDE_NONMATCH, _lib.SIDE_GENESTATS, _lib.SIDE_READSTATS]
    assert lib.musc_abi_version() == 3  # additions only


def test_wrappers_raise_when_the_library_refuses(lib):
    """Every entry point refuses a NULL context with code 1; the wrappers turn that into MuscatoError."""
    nb = ctypes.c_uint64(7)
    assert lib.musc_side_prepare(None, None, None) == 1
    assert lib.musc_side_text(None, 0, 0, 1, None, 0, 0, ctypes.byref(nb)) == 1
    assert lib.musc_side_last_ms(None, None, None) == 1
    e = Engine.__new__(Engine)  # no context: what a closed Engine holds
    e._lib, e._h = lib, None
    for call in (e.side_prepare, e.nonmatch_text, e.genestats_text, e.readstats_text, e.side_ms, lambda: e.readstats_text(3, 4)):
        with pytest.raises(MuscatoError, match=r"musc_side_\w+ failed \(1\)"):
            call()
