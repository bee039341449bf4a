"""raytracer_challenge_amd/cabi.py is the one ctypes mirror of include/rtc.h and include/rtw.h.  Nothing compiles it against the headers,
so it is held to them textually, the way test_shim_layout.py holds the Rust shim: every struct field for field, every prototype
parameter for parameter, and the table against the dynamic symbols of the libraries it is bound to."""
import ctypes as C
import os
import re
import subprocess

import pytest

import test_shim_layout
from raytracer_challenge_amd import cabi
from raytracer_challenge_amd.backend import Backend
from test_shim_layout import c_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = os.path.join(ROOT, "raytracer_challenge_amd", "csrc", "librtc_amd.so")
HEADERS = {h: open(os.path.join(ROOT, "include", h)).read() for h in ("rtc.h", "rtw.h")}
SCALARS = {"u64": C.c_uint64, "u32": C.c_uint32, "i32": C.c_int32, "f64": C.c_double, "c_int": C.c_int, "f32": C.c_float}   # c_struct's spellings
C_SCALARS = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int32_t": C.c_int32, "double": C.c_double, "int": C.c_int, "size_t": C.c_size_t,
             "uint8_t": C.c_uint8}
POINTER_KINDS = (C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p))


def struct_names(text):
    return re.findall(r"typedef struct (\w+)\s*\{", text)


def is_pointer(ctype):
    return ctype in POINTER_KINDS or issubclass(ctype, C._Pointer)


# ---- structs -------------------------------------------------------------------------------------------------------------------------
def test_every_struct_of_the_headers_has_one_mirror():
    names = [n for text in HEADERS.values() for n in struct_names(text)]
    assert len(names) >= 28 and sorted(names) == sorted(cabi.STRUCTS)                  # none left out, none invented
    assert len(set(cabi.STRUCTS.values())) == len(cabi.STRUCTS)                        # one class each
    mirrors = [v for v in vars(cabi).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure]
    assert sorted(map(id, set(mirrors))) == sorted(map(id, cabi.STRUCTS.values()))     # and no Structure beside them


@pytest.mark.parametrize("name", sorted(cabi.STRUCTS))
def test_struct_mirrors_the_header(name, monkeypatch):
    text = next(t for t in HEADERS.values() if name in struct_names(t))
    for nested in cabi.STRUCTS:   # a struct held by value parses as its own name (rtc_adaptive nests two rtc_sampling records)
        monkeypatch.setitem(test_shim_layout.C_TO_RUST, nested, nested)
    want, mirror = c_struct(text, name), cabi.STRUCTS[name]
    got = mirror._fields_
    assert [f[0] for f in got] == [f[0] for f in want]                                 # names and order
    offset, align = 0, 1
    for (field, kind, length), (_, ctype) in zip(want, got):
        elem = ctype._type_ if length else ctype
        assert (getattr(ctype, "_length_", 0) if length else 0) == length, (name, field)
        if kind == "ptr":
            assert is_pointer(elem), (name, field, elem)
        elif kind in cabi.STRUCTS:
            assert elem is cabi.STRUCTS[kind], (name, field, elem)
        else:
            assert elem is SCALARS[kind], (name, field, elem)
        a = C.alignment(elem)                                                          # the header's natural layout: each field at its own alignment
        offset = (offset + a - 1) // a * a
        assert getattr(mirror, field).offset == offset, (name, field)
        offset, align = offset + C.sizeof(ctype), max(align, a)
    assert C.sizeof(mirror) == (offset + align - 1) // align * align, name


# ---- prototypes ----------------------------------------------------------------------------------------------------------------------
def prototypes(text):
    """{name: (return type, [parameter types])} of a header, types as C spells them without `const` and parameter names."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"typedef struct \w+\s*\{.*?\}\s*\w+\s*;|enum\s*\{.*?\}\s*;|#[^\n]*", "", text, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(rt[cw]_\w+)\s*\(([^)]*)\)\s*;", text):
        types = []
        for p in [] if params.strip() == "void" else params.split(","):
            p = re.sub(r"\bconst\b", "", p)
            array = "[" in p
            p = re.sub(r"\[.*", "", p).strip()
            m = re.match(r"^(\w+)((?:\s*\*)*)\s*(\w*)$", p)
            assert m, (name, p)
            base, stars = m.group(1), m.group(2).replace(" ", "")
            types.append(base + stars + ("*" if array else ""))
        out[name] = ("".join(re.sub(r"\bconst\b", "", ret).split()), types)
    return out


PROTOS = {name: sig for text in HEADERS.values() for name, sig in prototypes(text).items()}


def check(ctype, c_type, where):
    if c_type == "void":
        assert ctype is None, where
    elif c_type == "char*":
        assert ctype is C.c_char_p, where
    elif c_type.endswith("*"):
        assert is_pointer(ctype), where             # one of the three pointer kinds (or a C string)
        if ctype not in POINTER_KINDS:
            assert c_type.count("*") == 1 and ctype._type_ is cabi.STRUCTS[c_type[:-1]], where
        if ctype is C.POINTER(C.c_void_p):
            assert c_type.count("*") == 2, where                                       # a pointer to a handle
        if c_type.count("*") == 2:
            assert ctype is C.POINTER(C.c_void_p), where
    else:
        assert ctype is C_SCALARS[c_type], where


def test_the_headers_declare_what_is_expected():
    assert len(PROTOS) >= 97 and "rtc_render" in PROTOS and "rtw_render" in PROTOS, len(PROTOS)   # the parser reads them all
    assert PROTOS["rtc_render_shutter"][1][:3] == ["rtc_scene**", "rtc_camera*", "uint32_t"] and PROTOS["rtw_last_error"] == ("char*", [])


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_prototype_has_its_row(name):
    ret, params = PROTOS[name]
    assert name in cabi.SIGNATURES, name
    restype, argtypes = cabi.SIGNATURES[name]
    assert len(argtypes) == len(params), (name, params)
    check(restype, ret, (name, "returns"))
    for k, (ctype, c_type) in enumerate(zip(argtypes, params)):
        check(ctype, c_type, (name, k, c_type))


# ---- exports -------------------------------------------------------------------------------------------------------------------------
def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return sorted(set(re.findall(r"\b(rt[cw]_\w+)$", out, re.M)))


def is_set(lib, name):
    res, args = cabi.SIGNATURES[name]
    fn = getattr(lib, name)
    return fn.restype is res and fn.argtypes == list(args)


def test_the_product_library_and_the_table_cover_each_other():
    names = exported(PRODUCT)
    assert len(names) >= len(PROTOS)
    assert [n for n in names if n not in cabi.SIGNATURES] == []                        # every dynamic symbol has a row
    assert [n for n in PROTOS if n not in names] == []                                 # every prototype is exported
    lib = cabi.load(PRODUCT)
    assert [n for n in names if not is_set(lib, n)] == []


def test_the_emulator_and_the_oracle_bind_their_subsets(orc):
    from emu_lib import emu
    for be in (emu(), orc):
        names = [n for n in exported(be.path) if n in cabi.SIGNATURES]
        assert len(names) >= 18 and set(names) < set(cabi.SIGNATURES)                  # a proper subset: rtw.h's core at the least
        assert cabi.bind(be.lib) is be.lib
        assert [n for n in names if not is_set(be.lib, n)] == []
        assert [n for n in exported(be.path) if n not in cabi.SIGNATURES] == []


def test_bind_once_is_enough():
    be = Backend(PRODUCT)
    assert be.lib is not be._lib                                                       # the callers' handle and the package's own
    for lib in (be.lib, be._lib):
        for _ in range(2):
            assert cabi.bind(lib) is lib
            for name, (res, args) in cabi.SIGNATURES.items():
                if hasattr(lib, name):
                    assert getattr(lib, name).argtypes == list(args) and getattr(lib, name).restype is res, name


def test_a_callers_argtypes_do_not_reach_the_package():
    """What callers of the raw entry points assign on Backend.lib (bench.py types rtc_render itself) leaves the package's calls alone."""
    be = Backend(PRODUCT)
    be.lib.rtw_make_camera.argtypes = [C.c_void_p, C.c_void_p]
    from raytracer_challenge_amd import scenes
    cam = scenes.cover(8, 4)[0]
    rc = be._rtc_camera(cam)
    assert isinstance(rc, cabi.RtcCameraC) and (rc.hsize, rc.vsize) == (8, 4)
    assert be._lib.rtw_make_camera.argtypes == list(cabi.SIGNATURES["rtw_make_camera"][1])
