"""include/muscato_hip.h as the ABI tests read it (no GPU, no library): the text without comments, the prototypes, the
integer constants, the fields of the structs, and their layout as a C compiler sees it.  The one reader of the header:
the test files ask this module and keep no regular expression or C program of their own."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "muscato_hip.h")
# the scalar C types the header uses -> their ctypes image
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint8_t": ctypes.c_uint8, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double, "char": ctypes.c_char}


def strip_comments(src, line_comments=False):
    """C text without its /* */ comments (line_comments: nor its // ones), each replaced by a blank."""
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src) if line_comments else src


@functools.lru_cache(maxsize=None)
def text():
    """The header without comments."""
    with open(HEADER) as f:
        return strip_comments(f.read())


def _squeeze(decl):
    """One declaration on one line, with single blanks."""
    return re.sub(r"\s+", " ", decl).strip()


@functools.lru_cache(maxsize=None)
def prototypes():
    """[(restype, name, [parameter declaration, ...]), ...] in the header's order; restype is "int", "void" or
    "const char*", a `(void)` list is empty."""
    out = []
    for ret, name, args in re.findall(r"^\s*(int|void|const char\s*\*)\s+(musc_\w+)\s*\(([^)]*)\)\s*;", text(), flags=re.M):
        params = [_squeeze(a) for a in args.split(",")]
        out.append((_squeeze(ret).replace(" *", "*"), name, [] if params == ["void"] else params))
    return out


def prototype(name):
    """(restype, [parameter declaration, ...]) of one entry point."""
    found = [(r, p) for r, n, p in prototypes() if n == name]
    assert len(found) == 1, name
    return found[0]


@functools.lru_cache(maxsize=None)
def constants():
    """{name: value} of the integer constants: `#define NAME 123` / `123u`, and the enumerators of the enums."""
    out = {n: int(v) for n, v in re.findall(r"^\s*#\s*define\s+(\w+)\s+(\d+)[uU]?\s*$", text(), flags=re.M)}
    for body in re.findall(r"\benum\s*\w*\s*\{([^}]*)\}", text()):
        for n, v in re.findall(r"(\w+)\s*=\s*(\d+)", body):
            out[n] = int(v)
    return out


@functools.lru_cache(maxsize=None)
def structs():
    """{struct name: [(field, C type, array length or None), ...]} of every `typedef struct {...} name;`, fields in
    the declared order; a pointer's type ends in `*`, an array length may be a constant's name."""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", text(), flags=re.S):
        fields = []
        for decl in filter(None, (_squeeze(d) for d in body.split(";"))):
            ctype, declarators = decl.split(" ", 1)
            for d in declarators.split(","):
                m = re.fullmatch(r"\s*(\**)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", d)
                assert m, decl
                n = m.group(3)
                fields.append((m.group(2), ctype + m.group(1), None if n is None else constants()[n] if n in constants() else int(n)))
        out[name] = fields
    return out


def struct_fields(name):
    return structs()[name]


@functools.lru_cache(maxsize=None)
def _layouts():
    """One C99 program over every struct of the header, compiled and run once per session."""
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "muscato_hip.h"\nint main(void) {\n'
    for s, fields in structs().items():
        src += '  printf("%s sizeof %%zu 0\\n", sizeof(%s));\n' % (s, s)
        for f, _, _ in fields:
            src += '  printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));\n' % (s, f, s, f, s, f)
    src += "  return 0;\n}\n"
    tmp = tempfile.mkdtemp(prefix="abi_layout_")
    try:
        with open(os.path.join(tmp, "layout.c"), "w", encoding="ascii") as f:
            f.write(src)
        exe = os.path.join(tmp, "layout")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", exe, os.path.join(tmp, "layout.c")])
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = {s: {"sizeof": None, "fields": {}} for s in structs()}
    for s, f, a, b in (line.split() for line in lines):
        if f == "sizeof":
            out[s]["sizeof"] = int(a)
        else:
            out[s]["fields"][f] = (int(a), int(b))
    return out


def c_layout(struct_names):
    """{struct: {"sizeof": bytes, "fields": {field: (offsetof, size of the field)}}} for the named structs, as printed
    by a C99 program that includes the header (gcc -std=c99 -Wall -Werror)."""
    return {s: _layouts()[s] for s in struct_names}
