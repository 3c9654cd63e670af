"""What the C ABI tests share: include/*.h read as data (structs, prototypes, integer macros), the loaded
library, the zeroed block that stands in for a context where an entry refuses before it looks into one,
the errno values, and the walk that shows an entry's checks come in their stated order."""
import ctypes as C
import functools
import glob
import os
import re

import pytest

from minimodem_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV, ERANGE, ENOTSUP = -22, -19, -34, -95
BASE = 1 << 20                                      # 16-byte aligned; never dereferenced

# C scalar type -> (kind, bytes) on the one ABI the library is built for (x86-64 Linux, LP64)
SCALARS = {"char": ("signed", 1), "int": ("signed", 4), "long": ("signed", 8), "long long": ("signed", 8),
           "unsigned": ("unsigned", 4), "unsigned int": ("unsigned", 4), "unsigned long long": ("unsigned", 8),
           "float": ("float", 4), "double": ("float", 8), "size_t": ("unsigned", 8)}
for _bits in (8, 16, 32, 64):
    SCALARS["int%d_t" % _bits] = ("signed", _bits // 8)
    SCALARS["uint%d_t" % _bits] = ("unsigned", _bits // 8)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def fake_ctx():
    buf = C.create_string_buffer(1 << 16)
    return C.cast(buf, C.c_void_p), buf


@functools.lru_cache(None)
def _headers():
    """include/*.h in one string, comments removed"""
    text = "".join(open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))))
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@functools.lru_cache(None)
def header_constants():
    """{name: value} of every `#define MIFSK_X <integer>`: decimal or hex, with or without the u, in
    parentheses or not, negative or not"""
    found = re.findall(r"^#define\s+(MIFSK_\w+)\s+\(?\s*(-?(?:0[xX][0-9a-fA-F]+|\d+))[uU]?\s*\)?\s*$", _headers(), re.M)
    return {name: int(value, 0) for name, value in found}


def _count(expr):
    """an array bound: an integer expression over the header's macros"""
    expr = re.sub(r"MIFSK_\w+", lambda m: str(header_constants()[m.group(0)]), expr)
    assert re.fullmatch(r"[\d\s+*()-]+", expr), expr
    return int(eval(expr))


def _layout(fields, structs):
    """(sizeof, alignment) of a struct of these fields under natural alignment"""
    end, most = 0, 1
    for _name, kind, size, count in fields:
        align = _layout(structs[kind[7:]], structs)[1] if kind.startswith("struct ") else size
        end = -(-end // align) * align + size * count
        most = max(most, align)
    return -(-end // most) * most, most


def header_sizeof(name):
    """sizeof(struct name) as the header's fields lay it out"""
    return _layout(header_structs()[name], header_structs())[0]


@functools.lru_cache(None)
def header_structs():
    """{struct name: [(field, kind, bytes, count)]} of every struct the headers give a body: kind is
    "pointer", "float", "signed", "unsigned" or "struct <name>", bytes the width of one element and count
    the array bound (1: no array).  `a, b[2]` after one type gives two fields."""
    structs = {}
    for name, body in re.findall(r"\bstruct\s+(\w+)\s*\{([^{}]*)\}", _headers()):
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            first, *others = [d.strip() for d in decl.split(",")]
            ctype, first = re.fullmatch(r"(.*?)(\**\s*\w+\s*(?:\[[^\]]*\])?)", first).groups()
            ctype = " ".join(w for w in ctype.replace("*", " * ").split() if w != "const")
            for declarator in [first] + others:
                stars, field, bound = re.fullmatch(r"(\**)\s*(\w+)\s*(?:\[([^\]]*)\])?", declarator).groups()
                if stars or ctype.endswith("*"):
                    kind, size = "pointer", 8
                elif ctype in SCALARS:
                    kind, size = SCALARS[ctype]
                else:
                    kind, size = "struct " + ctype, _layout(structs[ctype], structs)[0]
                fields.append((field, kind, size, _count(bound) if bound else 1))
        structs[name] = fields
    return structs


@functools.lru_cache(None)
def header_functions():
    """{function name: (return kind, argument count)} of every prototype: the kind is "void", "int", "float",
    "double", "long", "unsigned", "u64" (size_t, uint64_t) or "pointer" """
    text = re.sub(r"^\s*#.*$", "", _headers(), flags=re.M)
    functions = {}
    for ret, name, args in re.findall(r"([\w\s*]+?)\b((?:mifsk|fsk)_\w+)\s*\(([^()]*)\)\s*;", text):
        ret = " ".join(w for w in ret.split() if w != "const")
        kind = "pointer" if "*" in ret else {"size_t": "u64", "uint64_t": "u64"}.get(ret, ret)
        assert kind in ("void", "int", "float", "double", "long", "unsigned", "u64", "pointer"), (name, ret)
        functions[name] = (kind, 0 if args.strip() == "void" else args.count(",") + 1)
    return functions


def ladder(rc, late, order):
    """the earlier checks win over the later ones: with `late` as the one late violation, each earlier one
    alone still refuses, and so does every pair in the stated order"""
    for i, early in enumerate(order):
        assert rc(**dict(late, **early)) == EINVAL, early
        for later in order[i + 1:]:
            assert rc(**dict(late, **dict(later, **early))) == EINVAL, (early, later)
    assert rc(ctx=None, **late) == EINVAL
