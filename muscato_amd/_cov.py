"""The binding of include/muscato_cov.h (coverage): a prototype table of its own, in the header's order.
_lib.PROTOTYPES stays the image of include/muscato_hip.h alone; tests/test_cov_abi.py holds this table to the new header."""
from __future__ import annotations

import ctypes

from . import _lib

_int, _u32, _u64, _f32 = ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float
_vp, _P = ctypes.c_void_p, ctypes.POINTER

PROTOTYPES = {
    "musc_cov_prepare": (_int, [_vp, _u32, _P(_u64), _P(_u64), _P(_u64), _P(_u64)]),
    "musc_cov_text": (_int, [_vp, _int, _u64, _u64, _vp, _u64, _int, _P(_u64)]),
    "musc_cov_last_ms": (_int, [_vp, _P(_f32), _P(_f32)]),
}
SYMBOLS = list(PROTOTYPES)

# the flags of musc_cov_prepare
COV_REV_PAIRS, COV_WEIGHTED, COV_UNIQUE = 1, 2, 4
# `which` of musc_cov_text
COV_BEDGRAPH, COV_SUMMARY = 0, 1

_bound = None


def bind() -> ctypes.CDLL:
    """The loaded library with the coverage entry points typed; raises (never falls back) when one is not exported."""
    global _bound
    if _bound is not None:
        return _bound
    lib = _lib.load()
    for name, (restype, argtypes) in PROTOTYPES.items():
        if not hasattr(lib, name):
            raise ImportError("muscato_amd: %s does not export %s" % (_lib.LIB_PATH, name))
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    _bound = lib
    return lib
