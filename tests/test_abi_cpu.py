"""The whole C-ABI binding against include/mzsearch.h: muax_amd/_lib.py states every struct (STRUCTS) and every entry
point (ENTRIES) once, and this file compares both tables with the header -- names and order by reading the header's
plain declarations, every struct's size and every field's offset, size and kind by compiling the header with the host
C++ compiler.  No GPU, no kernel; the library is loaded only to see that load() applied the table."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from muax_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"float": C.c_float, "double": C.c_double, "int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64,
           "uint8_t": C.c_uint8, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "const char *": C.c_char_p}


# ---- the header, read as text: its declarators are a type, an optional const / *, a name, an optional [n] ----
def _header():
    text = open(os.path.join(ROOT, "include", "mzsearch.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))


STRUCT_RE = re.compile(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(mzs_\w+)\s*;", re.S)


def header_structs():
    """[(C name, [member names in order])] of every `typedef struct { ... } mzs_*;` (the opaque mzs_handle has no body)."""
    out = []
    for body, name in STRUCT_RE.findall(_header()):
        members = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            for piece in decl.split(","):  # `const float *a, *b` / `mzs_ez_head r, v, p` / `uint32_t key[2]`
                members.append(re.search(r"(\w+)\s*(?:\[\d+\])?$", piece.strip()).group(1))
        out.append((name, members))
    return out


def header_functions():
    """[(name, return type, [(base type, pointer depth, array length or None)])] of every function, in order."""
    text = STRUCT_RE.sub(" ", _header())
    found = re.findall(r"\b(const char \*|int64_t|int)\s*(mzs_\w+)\s*\(([^)]*)\)\s*;", text)
    assert len(found) == len(re.findall(r"\bmzs_\w+\s*\(", text)), "a declaration this reader does not understand"
    out = []
    for ret, name, params in found:
        parsed = []
        for p in filter(lambda p: p not in ("", "void"), (" ".join(p.split()) for p in params.split(","))):
            base, stars, _, length = re.fullmatch(r"(?:const )?(\w+) ?(\**) ?(\w+)(?:\[(\d+)\])?", p).groups()
            parsed.append((base, len(stars), int(length) if length else None))
        out.append((name, ret, parsed))
    return out


# ---- the header, as the compiler sees it ----
def _kind(t):
    """A ctypes type as the layout program spells it: p8, f4, i4, u4[2], s56 (a nested struct of 56 bytes)."""
    if issubclass(t, C.Array):
        return f"{_kind(t._type_)}[{t._length_}]"
    if issubclass(t, C.Structure):
        return f"s{C.sizeof(t)}"
    if t is C.c_void_p or issubclass(t, C._Pointer):
        return f"p{C.sizeof(t)}"
    letter = "f" if t in (C.c_float, C.c_double) else "u" if t(-1).value > 0 else "i"
    return f"{letter}{C.sizeof(t)}"


PROGRAM_HEAD = """#include <cstddef>
#include <cstdio>
#include <string>
#include <type_traits>
#include "mzsearch.h"
template <class T> std::string kind() {
  if (std::is_array<T>::value)
    return kind<typename std::remove_extent<T>::type>() + "[" + std::to_string(std::extent<T>::value) + "]";
  const char *k = std::is_pointer<T>::value ? "p" : std::is_floating_point<T>::value ? "f"
                  : std::is_integral<T>::value ? (std::is_signed<T>::value ? "i" : "u") : "s";
  return k + std::to_string(sizeof(T));
}
int main() {
"""


@pytest.fixture(scope="session")
def compiled_layout(tmp_path_factory):
    """{C name: (sizeof, {field: (offset, size, kind)})} for every struct and ctypes field of _lib.STRUCTS: ONE program,
    compiled once.  A field the header does not have is a compile error."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    lines = []
    for c_name, cls in _lib.STRUCTS.items():
        lines.append(f'  std::printf("{c_name} . %zu 0 -\\n", sizeof({c_name}));')
        for field, _ in cls._fields_:
            lines.append(f'  std::printf("{c_name} {field} %zu %zu %s\\n", offsetof({c_name}, {field}), '
                         f'sizeof((({c_name} *)0)->{field}), kind<decltype({c_name}::{field})>().c_str());')
    tmp = tmp_path_factory.mktemp("abi")
    src, exe = tmp / "layout.cpp", str(tmp / "layout")
    src.write_text(PROGRAM_HEAD + "\n".join(lines) + "\n  return 0;\n}\n")
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout
    layout = {c_name: [None, {}] for c_name in _lib.STRUCTS}
    for c_name, field, a, b, kind in (line.split() for line in out.splitlines()):
        if field == ".":
            layout[c_name][0] = int(a)
        else:
            layout[c_name][1][field] = (int(a), int(b), kind)
    return layout


# ---- the tests ----
def test_abi_version_is_1():
    assert re.search(r"#define MZS_ABI_VERSION 1\b", open(os.path.join(ROOT, "include", "mzsearch.h")).read())
    assert _lib.load(build_if_missing=True).mzs_abi_version() == 1


def test_structs_are_the_headers_in_its_order():
    names = [name for name, _ in header_structs()]
    assert "mzs_handle" not in names and len(set(names)) == len(names)
    assert list(_lib.STRUCTS) == names
    assert len(set(_lib.STRUCTS.values())) == len(_lib.STRUCTS)


def test_every_header_member_is_a_ctypes_field_in_the_same_order():
    for name, members in header_structs():
        assert [n for n, _ in _lib.STRUCTS[name]._fields_] == members, name


def test_every_struct_has_the_compilers_layout(compiled_layout):
    fields = 0
    for c_name, cls in _lib.STRUCTS.items():
        size, members = compiled_layout[c_name]
        assert C.sizeof(cls) == size, c_name
        for field, ctype in cls._fields_:
            d = getattr(cls, field)
            assert (d.offset, d.size, _kind(ctype)) == members[field], (c_name, field)
            if issubclass(ctype, C.Structure):  # a nested struct is one of the table's own
                assert ctype in _lib.STRUCTS.values(), (c_name, field)
        fields += len(cls._fields_)
    print(f"{len(_lib.STRUCTS)} structs, {fields} fields agree with the compiler")


def _accepts(argtype, base, stars, length):
    """Is `argtype` the declared type of a parameter `base [*...] name [length]`?"""
    if not stars and length is None:
        return argtype is SCALARS[base]
    if base in _lib.STRUCTS:
        return stars == 1 and argtype is C.POINTER(_lib.STRUCTS[base])
    if base == "mzs_handle" and stars == 2:
        return argtype is C.POINTER(C.c_void_p)
    if argtype is C.c_void_p:  # device pointers, handles and streams travel as integers
        return True
    if base not in SCALARS or stars + (length is not None) != 1 or not issubclass(argtype, C._Pointer):
        return False
    array = argtype._type_  # POINTER(element * n): n is the header's where it states one
    return issubclass(array, C.Array) and array._type_ is SCALARS[base] and length in (None, array._length_)


def test_entries_are_the_headers_functions_with_its_types():
    functions = header_functions()
    assert list(_lib.ENTRIES) == [name for name, _, _ in functions] and _lib.EXPORTED_SYMBOLS == list(_lib.ENTRIES)
    for name, ret, params in functions:
        restype, argtypes = _lib.ENTRIES[name]
        assert restype is RETURNS[ret], name
        assert isinstance(argtypes, list) and len(argtypes) == len(params), name
        for i, (argtype, param) in enumerate(zip(argtypes, params)):
            assert _accepts(argtype, *param), (name, i, param)
    print(f"{len(functions)} entries agree with the header")


def test_load_applies_the_table_to_every_entry():
    L = _lib.load(build_if_missing=True)
    for name, (restype, argtypes) in _lib.ENTRIES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
