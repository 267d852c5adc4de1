"""The SAM entry points (include/muscato_sam.h) without a GPU: the library exports them, the table of
muscato_amd/_sam.py states the new header prototype for prototype and type for type, the old header and its table are
what they were, and the Python methods exist."""
import ctypes
import inspect
import os
import re

from muscato_amd import _lib, _sam, api, build as mbuild

import abi_header as ah
from test_abi import RESTYPES, bindings_of

SAM_HEADER = os.path.join(ah.INCLUDE, "muscato_sam.h")
NAMES = ["musc_sam_prepare", "musc_sam_text", "musc_sam_last_ms"]


def sam_text():
    with open(SAM_HEADER) as f:
        return ah.strip_comments(f.read())


def sam_prototypes():
    """As abi_header.prototypes(), over the new header's text."""
    out = []
    for ret, name, args in re.findall(r"^\s*(int|void|const char\s*\*)\s+(musc_\w+)\s*\(([^)]*)\)\s*;", sam_text(), flags=re.M):
        params = [ah._squeeze(a) for a in args.split(",")]
        out.append((ah._squeeze(ret).replace(" *", "*"), name, [] if params == ["void"] else params))
    return out


def test_the_header_declares_three_entry_points_and_nothing_else():
    assert [n for _, n, _ in sam_prototypes()] == NAMES
    text = sam_text()
    assert '#include "muscato_hip.h"' in text and "typedef" not in text and "struct" not in text
    assert not re.search(r"#\s*define\s+MUSC_ABI_VERSION", text)
    assert SAM_HEADER in mbuild.HEADERS and os.path.join(mbuild.CSRC, "sam_plan.hpp") in mbuild.HEADERS
    assert os.path.join(mbuild.CSRC, "kernels_sam.hpp") in mbuild.HEADERS


def test_the_old_header_and_table_are_untouched():
    old = [n for _, n, _ in ah.prototypes()]
    assert len(old) == 58 and not set(old) & set(NAMES)
    assert _lib.SYMBOLS == old and not set(_lib.PROTOTYPES) & set(_sam.PROTOTYPES)


def test_the_library_exports_them():
    mbuild.build()
    lib = _sam.bind()
    for s in NAMES:
        assert hasattr(lib, s) and getattr(lib, s).restype is ctypes.c_int and getattr(lib, s).argtypes is not None
    assert lib.musc_abi_version() == 3


def test_the_binding_is_the_header_type_for_type():
    lib = _sam.bind()
    assert list(_sam.PROTOTYPES) == _sam.SYMBOLS == NAMES
    for ret, name, params in sam_prototypes():
        for restype, argtypes in (_sam.PROTOTYPES[name], (getattr(lib, name).restype, getattr(lib, name).argtypes)):
            assert restype is RESTYPES[ret], name
            assert len(argtypes) == len(params), name
            for decl, ct in zip(params, argtypes):
                assert ct in bindings_of(decl), "%s: `%s` bound as %s" % (name, decl, ct)
                if "*" not in decl and "uint64_t" in decl:
                    assert ctypes.sizeof(ct) == 8
    # scalar out-parameters only
    for _, name, params in sam_prototypes():
        for decl in params[1:]:
            assert decl.replace("*", " ").split()[0] in ("int", "uint64_t", "float", "char"), decl


def test_the_python_methods():
    for m, params in (("sam_prepare", ["self", "rev_pairs"]), ("sam_header", ["self"]), ("sam_text", ["self", "rec0", "nrec"]),
                      ("sam_ms", ["self"])):
        assert list(inspect.signature(getattr(api.Engine, m)).parameters) == params, m
    sig = inspect.signature(api.Engine.sam_prepare)
    assert sig.parameters["rev_pairs"].default is False
    sig = inspect.signature(api.Engine.sam_text)
    assert sig.parameters["rec0"].default == 0 and sig.parameters["nrec"].default is None


def test_a_null_context_is_an_error_not_a_fault():
    lib = _sam.bind()
    n = ctypes.c_uint64(7)
    assert lib.musc_sam_prepare(None, 0, ctypes.byref(n), None, None) == 1
    assert lib.musc_sam_text(None, 1, 0, 1, None, 0, 0, ctypes.byref(n)) == 1
    assert lib.musc_sam_last_ms(None, None, None) == 1
