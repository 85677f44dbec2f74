"""The binding is derived from include/navenv.h (nav/_abi.py): the reader on a synthetic header
that holds every construct the real one uses and on what it must refuse, the real header's counts,
and the derived ctypes layouts against the layouts the library's own host compiler gives the
header's structs. No GPU, no library load."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "navenv.h")

SYNTHETIC = """
/* a block comment; with a semicolon, a paren ( and a fake prototype:
 * int nav_fake(const float* x, void* stream);
 */
#ifndef T_H
#define T_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define NAV_ABI_VERSION 11
#define NAV_EINVAL (-100000)
#define NAV_ROW 8   /* trailing; comment ( */
#define NAV_CELLS 100 /* a comment that runs on
                         int nav_fake2(void); */
// int nav_fake3(void);
typedef struct nav_inner {
    int32_t d_in;   /* int nav_fake4(void); */
    float* params;
} nav_inner;
typedef struct nav_outer {
    nav_inner actor, critics[2], target;
    float *m_critic[2], *v_critic[2];
    double lr, lr2;
    const int64_t* idx;
    uint8_t flag;
    uint16_t* masks[2];
    uint32_t seed_lo, seed_hi;
    uint64_t* sums;
} nav_outer;
int nav_version(void);
void nav_defaults(nav_inner* p);
int64_t nav_count(int32_t a,
                  int64_t b);
int32_t nav_res(void);
int nav_forward(const nav_inner* nets, int32_t n, const float* in,
                float* const* out, const uint16_t* const* masks, double lr, float tau,
                uint32_t seed, const nav_outer* members, const float* step_size,
                nav_outer* scores, void** event, const void* table,
                void* stream);
#define NAV_LATE 16
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_every_construct():
    from nav import _abi
    defines, structs, protos = _abi.parse(SYNTHETIC)
    assert defines == {"NAV_ABI_VERSION": 11, "NAV_EINVAL": -100000, "NAV_ROW": 8,
                       "NAV_CELLS": 100, "NAV_LATE": 16}
    assert list(structs) == ["nav_inner", "nav_outer"]
    assert structs["nav_inner"] == [("d_in", "int32_t", 0, 0), ("params", "float", 1, 0)]
    assert structs["nav_outer"] == [
        ("actor", "nav_inner", 0, 0), ("critics", "nav_inner", 0, 2), ("target", "nav_inner", 0, 0),
        ("m_critic", "float", 1, 2), ("v_critic", "float", 1, 2),
        ("lr", "double", 0, 0), ("lr2", "double", 0, 0), ("idx", "int64_t", 1, 0),
        ("flag", "uint8_t", 0, 0), ("masks", "uint16_t", 1, 2),
        ("seed_lo", "uint32_t", 0, 0), ("seed_hi", "uint32_t", 0, 0), ("sums", "uint64_t", 1, 0)]
    assert list(protos) == ["nav_version", "nav_defaults", "nav_count", "nav_res", "nav_forward"]
    assert protos["nav_version"] == ("int", [])
    assert protos["nav_defaults"] == ("void", [("nav_inner*", "p")])
    assert protos["nav_count"] == ("int64_t", [("int32_t", "a"), ("int64_t", "b")])
    assert protos["nav_forward"] == ("int", [
        ("nav_inner*", "nets"), ("int32_t", "n"), ("float*", "in"), ("float**", "out"),
        ("uint16_t**", "masks"), ("double", "lr"), ("float", "tau"), ("uint32_t", "seed"),
        ("nav_outer*", "members"), ("float*", "step_size"), ("nav_outer*", "scores"),
        ("void**", "event"), ("void*", "table"), ("void*", "stream")])


def test_types_follow_from_the_parse_by_rule():
    from nav import _abi
    _, structs, protos = _abi.parse(SYNTHETIC)
    cls = _abi.struct_classes(structs, {"nav_inner": "Inner", "nav_outer": "Outer"})
    inner, outer = cls["nav_inner"], cls["nav_outer"]
    assert (inner.__name__, outer.__name__) == ("Inner", "Outer")
    assert inner._fields_ == [("d_in", C.c_int32), ("params", C.c_void_p)]
    assert outer._fields_ == [
        ("actor", inner), ("critics", inner * 2), ("target", inner),
        ("m_critic", C.c_void_p * 2), ("v_critic", C.c_void_p * 2),
        ("lr", C.c_double), ("lr2", C.c_double), ("idx", C.c_void_p), ("flag", C.c_uint8),
        ("masks", C.c_void_p * 2), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32),
        ("sums", C.c_void_p)]
    f32 = C.POINTER(C.c_float)
    sig = {s[0]: s[1:] for s in _abi.signatures(protos, cls, {
        ("nav_forward", "step_size"): f32, ("nav_forward", "scores"): C.c_void_p})}
    assert sig["nav_version"] == (C.c_int, [])
    assert sig["nav_defaults"] == (None, [C.POINTER(inner)])
    assert sig["nav_count"] == (C.c_int64, [C.c_int32, C.c_int64])
    assert sig["nav_res"] == (C.c_int32, [])
    pp = C.POINTER(C.c_void_p)
    assert sig["nav_forward"] == (C.c_int, [
        C.POINTER(inner), C.c_int32, C.c_void_p, pp, pp, C.c_double, C.c_float, C.c_uint32,
        C.POINTER(outer), f32, C.c_void_p, pp, C.c_void_p, C.c_void_p])


REFUSED = {
    "an unknown scalar type": "int nav_f(size_t n);",
    "an unknown member type": "typedef struct nav_s { long n; } nav_s;",
    "a struct used before its declaration":
        "int nav_f(const nav_s* s);\ntypedef struct nav_s { int32_t n; } nav_s;",
    "a function-pointer parameter": "int nav_f(int (*cb)(int), void* stream);",
    "a parameter without a name": "int nav_f(int32_t, void* stream);",
    "an array parameter": "int nav_f(float x[2]);",
    "a struct by value as a parameter":
        "typedef struct nav_s { int32_t n; } nav_s;\nint nav_f(nav_s s);",
    "a void member": "typedef struct nav_s { void x; } nav_s;",
    "a bit-field": "typedef struct nav_s { uint32_t a : 3; } nav_s;",
    "a two-dimensional array member": "typedef struct nav_s { float a[2][2]; } nav_s;",
    "a typedef under another name": "typedef struct nav_s { int32_t n; } nav_t;",
    "a pointer return": "const float* nav_f(void);",
    "a prototype without its semicolon": "int nav_f(void)\nint nav_g(void);",
    "a prototype of another prefix": "int other_f(void);",
    "a stray token between declarations": "int nav_f(void);\nstatic\nint nav_g(void);",
    "a prototype declared twice": "int nav_f(void);\nint nav_f(void);",
    "a define that is no integer": "#define NAV_X 1.5f",
    "a define without a value": "#define NAV_X",
    "a function-like define": "#define NAV_X(a) 3",
    "an unclosed extern block": 'extern "C" {\nint nav_f(void);',
}


@pytest.mark.parametrize("what", REFUSED)
def test_parser_refuses(what):
    from nav import _abi
    with pytest.raises(_abi.NavError):
        _abi.parse(REFUSED[what])


def test_struct_names_and_overrides_must_match_the_header():
    from nav import _abi
    _, structs, protos = _abi.parse(SYNTHETIC)
    names = {"nav_inner": "Inner", "nav_outer": "Outer"}
    with pytest.raises(_abi.NavError, match="nav_outer"):  # a header struct without a name
        _abi.struct_classes(structs, {"nav_inner": "Inner"})
    with pytest.raises(_abi.NavError, match="nav_gone"):   # a name without a header struct
        _abi.struct_classes(structs, dict(names, nav_gone="Gone"))
    cls = _abi.struct_classes(structs, names)
    for key in (("nav_forward", "step_sizes"), ("nav_forwards", "step_size"),
                ("nav_version", "stream")):
        with pytest.raises(_abi.NavError, match=key[1]):
            _abi.signatures(protos, cls, {key: C.c_void_p})


def test_missing_header_is_named():
    from nav import _abi
    with pytest.raises(_abi.NavError, match="/no/such/include/navenv.h"):
        _abi.parse_header("/no/such/include/navenv.h")
    assert _abi.HEADER == HEADER


def test_real_header_counts_and_what_follows_from_them():
    from nav import _abi, _lib
    import nav.config as K
    defines, structs, protos = _abi.parse_header()
    assert len(protos) == 95 and len(structs) == 10
    assert len(_lib.SIGNATURES) == 95 and [s[0] for s in _lib.SIGNATURES] == list(protos)
    assert set(_lib.STRUCT_NAMES) == set(structs)
    assert (_lib.ABI_VERSION, _lib.NAV_EINVAL) == (defines["NAV_ABI_VERSION"], -100000)
    assert K.NSTEP_MAX == defines["NAV_NSTEP_MAX"] == 16
    assert _lib._COUNT_FNS == {f for f, (ret, _) in protos.items() if ret.startswith("int")
                               and ret != "int"}
    assert len(_lib._COUNT_FNS) == 14 and len(_lib.ARG_OVERRIDES) == 14
    # a struct pointer is typed everywhere but where the override says it is a device buffer
    sig = {s[0]: s for s in _lib.SIGNATURES}
    assert sig["nav_act"][2][:2] == [C.POINTER(_lib.NavParams), C.POINTER(_lib.NavMlp)]
    assert sig["nav_pop_test_summary"][2] == [C.POINTER(_lib.NavTestOut), C.c_int32, C.c_int32,
                                              C.c_void_p, C.c_void_p]


SIZES = {"nav_params": 96, "nav_env_soa": 80, "nav_step_out": 32, "nav_replay": 16, "nav_mlp": 40,
         "nav_test_out": 40, "nav_pop_score": 32, "nav_per": 32, "nav_td3_member": 576,
         "nav_td3_member_bc": 48}


def host_compiler():
    """The compiler the Makefile builds libnavenv.so with (HIPCC ?= /opt/rocm/bin/hipcc)."""
    for cc in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cc and os.path.exists(cc):
            return cc
    pytest.fail("no hipcc: the layouts cannot be compared with the compiler's")


def test_layouts_equal_the_compilers(tmp_path):
    """sizeof of every struct and offsetof of every member, printed by a host-only program the
    library's compiler builds from the header, equal what ctypes gives the derived classes."""
    from nav import _abi, _lib
    structs = _abi.parse_header()[1]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "navenv.h"', 'int main(void) {']
    for s, fields in structs.items():
        lines.append(f'    printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'    printf("{s}.{f[0]} %zu\\n", offsetof({s}, {f[0]}));' for f in fields]
    lines += ['    return 0;', '}', '']
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([host_compiler(), "-x", "c++", "-std=c++17", "-O0",
                    "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    compiled = {k: int(n) for k, n in (line.split() for line in out.splitlines())}
    derived = {}
    for s, fields in structs.items():
        cls = getattr(_lib, _lib.STRUCT_NAMES[s])
        derived[s] = C.sizeof(cls)
        derived.update({f"{s}.{f[0]}": getattr(cls, f[0]).offset for f in fields})
    assert derived == compiled
    assert {s: derived[s] for s in structs} == SIZES
    assert len(derived) == 10 + 95  # ten sizes and the offsets of 95 members
