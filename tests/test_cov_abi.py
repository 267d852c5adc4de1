"""The coverage entry points (include/muscato_cov.h) without a GPU: the library exports them, the table of
muscato_amd/_cov.py states the new header prototype for prototype and type for type, the old header and its table are
what they were, and the Python methods exist."""
import ctypes
import inspect
import os
import re

from muscato_amd import _lib, _cov, api, build as mbuild

import abi_header as ah
from test_abi import RESTYPES, bindings_of

COV_HEADER = os.path.join(ah.INCLUDE, "muscato_cov.h")
NAMES = ["musc_cov_prepare", "musc_cov_text", "musc_cov_last_ms"]


def cov_header_text():
    with open(COV_HEADER) as f:
        return ah.strip_comments(f.read())


def cov_prototypes():
    """As abi_header.prototypes(), over the new header's text."""
    out = []
    for ret, name, args in re.findall(r"^\s*(int|void|const char\s*\*)\s+(musc_\w+)\s*\(([^)]*)\)\s*;", cov_header_text(), flags=re.M):
        params = [ah._squeeze(a) for a in args.split(",")]
        out.append((ah._squeeze(ret).replace(" *", "*"), name, [] if params == ["void"] else params))
    return out


def test_the_header_declares_three_entry_points_and_nothing_else():
    assert [n for _, n, _ in cov_prototypes()] == NAMES
    text = cov_header_text()
    assert '#include "muscato_hip.h"' in text and "typedef" not in text and "struct" not in text
    assert dict(re.findall(r"#\s*define\s+(MUSC_COV_\w+)\s+(\d+)u", text)) == {"MUSC_COV_REV_PAIRS": "1", "MUSC_COV_WEIGHTED": "2", "MUSC_COV_UNIQUE": "4"}
    assert (_cov.COV_REV_PAIRS, _cov.COV_WEIGHTED, _cov.COV_UNIQUE) == (1, 2, 4)
    assert not re.search(r"#\s*define\s+MUSC_ABI_VERSION", text)
    assert COV_HEADER in mbuild.HEADERS and os.path.join(mbuild.CSRC, "cov_plan.hpp") in mbuild.HEADERS
    assert os.path.join(mbuild.CSRC, "kernels_cov.hpp") in mbuild.HEADERS


def test_the_old_header_and_table_are_untouched():
    old = [n for _, n, _ in ah.prototypes()]
    assert len(old) == 58 and not set(old) & set(NAMES)
    assert _lib.SYMBOLS == old and not set(_lib.PROTOTYPES) & set(_cov.PROTOTYPES)


def test_the_library_exports_them():
    mbuild.build()
    lib = _cov.bind()
    for s in NAMES:
        assert hasattr(lib, s) and getattr(lib, s).restype is ctypes.c_int and getattr(lib, s).argtypes is not None
    assert lib.musc_abi_version() == 3


def test_the_binding_is_the_header_type_for_type():
    lib = _cov.bind()
    assert list(_cov.PROTOTYPES) == _cov.SYMBOLS == NAMES
    for ret, name, params in cov_prototypes():
        for restype, argtypes in (_cov.PROTOTYPES[name], (getattr(lib, name).restype, getattr(lib, name).argtypes)):
            assert restype is RESTYPES[ret], name
            assert len(argtypes) == len(params), name
            for decl, ct in zip(params, argtypes):
                assert ct in bindings_of(decl), "%s: `%s` bound as %s" % (name, decl, ct)
                if "*" not in decl and "uint64_t" in decl:
                    assert ctypes.sizeof(ct) == 8
    # scalar out-parameters only
    for _, name, params in cov_prototypes():
        for decl in params[1:]:
            assert decl.replace("*", " ").split()[0] in ("int", "uint32_t", "uint64_t", "float", "char"), decl


def test_the_python_methods():
    for m, params in (("cov_prepare", ["self", "rev_pairs", "weighted", "unique"]), ("cov_bedgraph", ["self", "rec0", "nrec"]),
                      ("cov_summary", ["self", "rec0", "nrec"]), ("cov_ms", ["self"])):
        assert list(inspect.signature(getattr(api.Engine, m)).parameters) == params, m
    sig = inspect.signature(api.Engine.cov_prepare)
    assert all(sig.parameters[k].default is False for k in ("rev_pairs", "weighted", "unique"))
    for m in ("cov_bedgraph", "cov_summary"):
        sig = inspect.signature(getattr(api.Engine, m))
        assert sig.parameters["rec0"].default == 0 and sig.parameters["nrec"].default is None


def test_a_null_context_is_an_error_not_a_fault():
    lib = _cov.bind()
    n = ctypes.c_uint64(7)
    assert lib.musc_cov_prepare(None, 0, ctypes.byref(n), None, None, None) == 1
    assert lib.musc_cov_text(None, 1, 0, 1, None, 0, 0, ctypes.byref(n)) == 1
    assert lib.musc_cov_last_ms(None, None, None) == 1
