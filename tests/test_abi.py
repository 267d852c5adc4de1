"""The C-ABI library loads and exports every symbol include/muscato_hip.h declares, and the Python binding
(muscato_amd/_lib.py) states that header exactly: every struct field for field against a compiled C program, every
prototype type for type (no GPU)."""
import ctypes
import os

import pytest

from muscato_amd import _lib, api, build as mbuild

import abi_header as ah

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {"musc_hit": _lib.MuscHit, "musc_params": _lib.MuscParams, "musc_stats": _lib.MuscStats,
           "musc_fastq_prep": _lib.MuscFastqPrep, "musc_read_names": _lib.MuscReadNames,
           "musc_db_text_info": _lib.MuscDbTextInfo, "musc_targets_prep_info": _lib.MuscTargetsPrepInfo}
SCALARS = ah.SCALARS
RESTYPES = {"int": ctypes.c_int, "void": None, "const char*": ctypes.c_char_p}


def test_library_builds_and_exports_header_symbols():
    mbuild.build()
    lib = _lib.load()
    declared = {name for _, name, _ in ah.prototypes()}
    assert declared == set(_lib.SYMBOLS), (declared ^ set(_lib.SYMBOLS))
    for s in declared:
        assert hasattr(lib, s), s
    assert lib.musc_abi_version() == 3


def test_symbols_are_the_header_prototypes_in_order():
    names = [name for _, name, _ in ah.prototypes()]
    assert len(names) == 58 and len(set(names)) == 58
    assert _lib.SYMBOLS == names
    assert list(_lib.PROTOTYPES) == names


def test_struct_layouts_match_header():
    assert ctypes.sizeof(_lib.MuscHit) == 16
    # n_windows + 16 windows + ww (+pad) + double + 6 ints + 5 reserved
    assert ctypes.sizeof(_lib.MuscParams) == 4 + 64 + 4 + 8 + 4 * 6 + 4 * 5 + 4
    assert ctypes.sizeof(_lib.MuscStats) == 8 * 8 + 2 * 4 + 8 * 4 + 8 + 2 * 4 + 4 * 8


def image(ctype, count=None):
    """The ctypes image of a C type of the header: a scalar, a struct by name, a pointer to either, an array."""
    if ctype.endswith("*"):
        return ctypes.POINTER(image(ctype[:-1]))
    t = STRUCTS[ctype] if ctype in STRUCTS else SCALARS[ctype]
    return t if count is None else t * count


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_struct_equals_the_header_field_for_field(name):
    """Names and order as declared, every field's type the image of its C type, and sizeof, every offsetof and every
    field's size what a C program that includes the header prints."""
    cls, declared = STRUCTS[name], ah.struct_fields(name)
    assert [f for f, _ in cls._fields_] == [f for f, _, _ in declared]
    for (f, bound), (_, ctype, count) in zip(cls._fields_, declared):
        assert bound is image(ctype, count), "%s.%s: `%s` bound as %s" % (name, f, ctype, bound)
    c = ah.c_layout([name])[name]
    assert ctypes.sizeof(cls) == c["sizeof"]
    assert {f: (getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_} == c["fields"]


def test_every_struct_of_the_header_is_bound():
    assert set(ah.structs()) == set(STRUCTS)


def test_init_without_gpu_fails_loudly():
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.musc_init(0, ctypes.byref(h))
    if rc == 0:  # a GPU is present: fine, clean up
        lib.musc_destroy(h)
        return
    msg = lib.musc_last_error(None).decode()
    assert "no CPU fallback" in msg or "gfx950" in msg or "HIP" in msg


def test_every_entry_point_has_matching_argtypes():
    """Each prototype of include/muscato_hip.h against the ctypes binding: same number of
    parameters, pointers bound as pointers, 64-bit integers as 64-bit.  A call through a binding
    without argtypes passes Python ints as 32-bit C ints: a pointer or a uint64 count is cut to
    its low half and the library then reads through a wild address on the host (the r01 SIGSEGV
    inside musc_reads_sort_unique, gpurun_out/t54.log: `offsets[nreads]` read through a
    truncated pointer).  This check needs no GPU."""
    lib = _lib.load()
    assert {n for _, n, _ in ah.prototypes()} == set(_lib.SYMBOLS)
    for _, name, params in ah.prototypes():
        at = getattr(lib, name).argtypes
        assert at is not None or not params, "%s: argtypes not declared" % name
        at = list(at or [])
        assert len(at) == len(params), "%s: %d parameters in the header, %d in the binding" % (name, len(params), len(at))
        for decl, ct in zip(params, at):
            is_ptr = "*" in decl
            bound_ptr = ct is ctypes.c_void_p or ct is ctypes.c_char_p or hasattr(ct, "contents") or \
                issubclass(ct, ctypes._Pointer)
            assert is_ptr == bound_ptr, "%s: `%s` bound as %s" % (name, decl, ct)
            if not is_ptr and "uint64_t" in decl:
                assert ctypes.sizeof(ct) == 8, "%s: `%s` bound as a %d-byte integer" % (name, decl, ctypes.sizeof(ct))


def bindings_of(decl):
    """The ctypes types a parameter declaration may be bound as.  A value: the type of the same C type.  A pointer:
    c_void_p, c_char_p for a `char*`, or POINTER(T), T the image of the pointee -- a struct by name, a scalar by type,
    c_void_p for a pointer to a pointer (an opaque musc_ctx has no image)."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    base, stars = words[0], words.count("*")
    assert words[-1] != "*" and len(words) == stars + 2, decl  # (type, stars, name)
    if not stars:
        return {SCALARS[base]}
    ok = {ctypes.c_void_p}
    if stars == 2:
        ok.add(ctypes.POINTER(ctypes.c_void_p))
    elif base != "musc_ctx":
        ok.add(ctypes.POINTER(image(base)))
        if base == "char":
            ok.add(ctypes.c_char_p)
    return ok


@pytest.mark.parametrize("where", ["table", "library"])
def test_every_prototype_is_bound_type_for_type(where):
    """All 58, with no exceptions list: restype c_int for int, None for void, c_char_p for const char*; every
    parameter one of bindings_of its declaration.  Held for the table of _lib.py and for what load() left on the
    functions of the library."""
    lib = _lib.load()
    assert len(ah.prototypes()) == 58
    for ret, name, params in ah.prototypes():
        if where == "table":
            restype, argtypes = _lib.PROTOTYPES[name]
        else:
            restype, argtypes = getattr(lib, name).restype, getattr(lib, name).argtypes
        assert restype is RESTYPES[ret], "%s: returns `%s`, restype %s" % (name, ret, restype)
        assert len(argtypes) == len(params), name
        for decl, ct in zip(params, argtypes):
            assert ct in bindings_of(decl), "%s: `%s` bound as %s" % (name, decl, ct)


def test_constants_are_the_header_defines():
    c = ah.constants()
    assert _lib.MUSC_MAX_WINDOWS == c["MUSC_MAX_WINDOWS"]
    kernels = {"MUSC_INST_MATCH_T": "k_match_t", "MUSC_INST_MATCH_G": "k_match_g", "MUSC_INST_SCREEN": "k_screen",
               "MUSC_INST_SCREEN_T": "k_screen_t", "MUSC_INST_CONFIRM": "k_confirm"}
    assert {k for k in c if k.startswith("MUSC_INST_")} == set(kernels)
    assert {fam: name for fam, (name, _) in api._INST_FIELDS.items()} == {c[k]: v for k, v in kernels.items()}
    assert api._INSTANCE_WORDS == c["MUSC_INSTANCE_WORDS"]
    seen = []

    class Lib:
        @staticmethod
        def musc_last_instance(h, out):
            seen.append(len(out))
            return 0
    e = api.Engine.__new__(api.Engine)
    e._lib, e._h = Lib, None
    assert e.last_instance()["path"] == "none" and seen == [c["MUSC_INSTANCE_WORDS"]]


def test_rccl_probe_reports_a_missing_library():
    """rccl_api() called dlerror() twice (the second call returns NULL) and built a
    std::string from it.  With the loader pointed at a file that does not exist the probe must come
    back with code 20 and the loader's message -- in a process of its own, the lookup is cached."""
    import subprocess
    import sys
    code = ("import ctypes\nfrom muscato_amd import _lib\nlib = _lib.load()\nbuf = ctypes.create_string_buffer(256)\n"
            "rc = lib.musc_rccl_probe(buf, 256)\nprint(rc, buf.value.decode())\n")
    env = dict(os.environ, MUSC_RCCL_LIB="/nonexistent/librccl.so.1", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rc, msg = out.stdout.strip().split(" ", 1)
    assert rc == "20" and "cannot load librccl" in msg and "nonexistent" in msg
