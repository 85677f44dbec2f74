"""Reader of include/navenv.h, the one statement of the C ABI: its NAV_* constants, structs and
prototypes, and the ctypes structures and signatures that follow from them by rule. Stdlib only
(config.py reads a constant through it without torch or a device). The grammar is the header's
own: integer defines, `typedef struct T { ... } T;` and `ret nav_name(params);`. Whatever else it
meets is an error, never a guess.
"""
import ctypes as C
import functools
import os
import re

HEADER = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..",
                                       "include", "navenv.h"))
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8,
           "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "float": C.c_float, "double": C.c_double}

_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(NAV_\w+)\b(.*)$", re.M)
_DECL = re.compile(r"\s*(?:typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;"
                   r"|([\w\s*]+?)\b(nav_\w+)\s*\(([^(){};]*)\)\s*;)")
_DECLARATOR = re.compile(r"((?:\* )*)(\w+)(?: \[(\d+)\])?")


class NavError(RuntimeError):
    pass


def _declarators(text, known):
    """`const T* const* a, b[2]` -> [(name, T, pointer depth, array length or 0), ...]"""
    toks = re.findall(r"\w+|\*|,|\[\d+\]", text)
    if "".join(toks) != "".join(text.split()) or not toks:
        raise NavError(f"navenv.h: cannot read the declaration {text.strip()!r}")
    base, *rest = [t for t in toks if t != "const"]
    if base not in known:
        raise NavError(f"navenv.h: unknown type {base!r} in {text.strip()!r}")
    out = []
    for d in " ".join(rest).split(","):
        m = _DECLARATOR.fullmatch(d.strip())
        if not m or (base == "void" and not m[1]):
            raise NavError(f"navenv.h: cannot split the declaration {text.strip()!r}")
        out.append((m[2], base, m[1].count("*"), int(m[3] or 0)))
    return out


def parse(text):
    """(defines {name: int}, structs {name: [(field, base type, pointer depth, array length or
    0)]}, prototypes {name: (return type, [(type, parameter)])}) of a header's text, each in
    declaration order; a parameter's type is its base type followed by one `*` per level."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {}
    for name, value in _DEFINE.findall(text):
        m = re.fullmatch(r"\(\s*(-?\d+)\s*\)|(-?\d+)", value.strip())
        if not m:
            raise NavError(f"navenv.h: #define {name} is not an integer: {value.strip()!r}")
        defines[name] = int(m[1] or m[2])
    body = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    body, n_extern = re.subn(r'extern\s+"C"\s*\{', "", body)
    structs, protos, pos = {}, {}, 0
    while m := _DECL.match(body, pos):
        pos = m.end()
        known = {"void", *SCALARS, *structs}
        if m[1]:
            if m[1] != m[3] or m[1] in structs:
                raise NavError(f"navenv.h: struct {m[1]} is declared twice or named {m[3]}")
            structs[m[1]] = [f for d in m[2].split(";") if d.strip()
                             for f in _declarators(d, known)]
            continue
        ret = m[4].strip()
        if ret not in ("void", *SCALARS) or m[5] in protos:
            raise NavError(f"navenv.h: {m[5]} returns {ret!r} or is declared twice")
        params = []
        for p in [] if m[6].strip() == "void" else m[6].split(","):
            (name, base, depth, n), = _declarators(p, known)
            if n or (base in structs and not depth):
                raise NavError(f"navenv.h: {m[5]} takes an array or a struct by value: "
                               f"{p.strip()!r}")
            params.append((base + "*" * depth, name))
        protos[m[5]] = (ret, params)
    if body[pos:].split() != ["}"] * n_extern:
        raise NavError(f"navenv.h: cannot read {body[pos:].strip()[:80]!r}")
    return defines, structs, protos


@functools.lru_cache(maxsize=None)
def parse_header(path=HEADER):
    """parse() of the header file, read once per process."""
    if not os.path.exists(path):
        raise NavError(f"{path} is missing: the binding is derived from it")
    with open(path) as f:
        return parse(f.read())


def struct_classes(structs, names):
    """{header name: ctypes.Structure} for `names` {header name: Python class name}, which must
    name exactly the header's structs. A pointer member is c_void_p, a scalar maps by type, a
    nested struct by value, an array is T * n."""
    if set(names) != set(structs):
        raise NavError(f"navenv.h structs without a Python name, or names without a struct: "
                       f"{sorted(set(names) ^ set(structs))}")
    classes = {}
    for cname, fields in structs.items():
        out = []
        for name, base, depth, n in fields:
            t = C.c_void_p if depth else classes.get(base) or SCALARS[base]
            out.append((name, t * n if n else t))
        classes[cname] = type(names[cname], (C.Structure,), {
            "_fields_": out, "__doc__": f"{cname} of include/navenv.h"})
    return classes


def signatures(protos, classes, overrides):
    """[(name, restype, argtypes)]: a scalar by type, a pointer to an ABI struct POINTER(Struct),
    any pointer to pointer POINTER(c_void_p), every other pointer c_void_p; `overrides`
    {(function, parameter): ctype} replaces single arguments and may name only what exists."""
    def ctype(t):
        base, depth = t.rstrip("*"), t.count("*")
        if depth > 1:
            return C.POINTER(C.c_void_p)
        if depth:
            return C.POINTER(classes[base]) if base in classes else C.c_void_p
        return SCALARS[base]
    stray = set(overrides) - {(fn, name) for fn, (_, ps) in protos.items() for _, name in ps}
    if stray:
        raise NavError(f"argument overrides that name no parameter of navenv.h: {sorted(stray)}")
    return [(fn, None if ret == "void" else SCALARS[ret],
             [overrides.get((fn, name), ctype(t)) for t, name in ps])
            for fn, (ret, ps) in protos.items()]
