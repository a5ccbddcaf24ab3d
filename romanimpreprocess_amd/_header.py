"""Parser of ``include/romanhip.h``: the C interface as Python objects, read from its one statement.

``parse(text)`` yields the constants (``#define NAME <integer>`` and enumerators), the structs as ``ctypes.Structure`` classes
and the prototypes with, per parameter, its name, its ``ctypes`` type and the element type of a pointer.  It reads the subset
of C the header confines itself to -- comments, the include guard, ``#include``, the ``__cplusplus`` block, ``typedef struct X
X;``, enums, ``typedef struct [tag] { fields } name;`` and ``ret name(params);`` over the fixed-width integer types, ``int``,
``unsigned``, ``size_t``, ``float``, ``double``, ``char`` and ``void`` -- and raises ``HeaderError`` naming the line on
anything else.  It never guesses.
"""

import ast
import ctypes as C
import re
from collections import namedtuple

SCALARS = {
    "int8_t": C.c_int8, "uint8_t": C.c_uint8, "int16_t": C.c_int16, "uint16_t": C.c_uint16, "int32_t": C.c_int32,
    "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "int": C.c_int, "unsigned": C.c_uint,
    "unsigned int": C.c_uint, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double, "char": C.c_char,
}

# name, ctypes type (the argtypes entry), C type as text (arrays decayed), pointer depth, pointee ("float", a struct's name, ...)
Param = namedtuple("Param", "name ctype ctext depth elem")
Proto = namedtuple("Proto", "name restype rettext params")
Header = namedtuple("Header", "constants structs prototypes opaque text")

_DECL = re.compile(r"\s*(?P<const>const\s+)?(?P<type>unsigned\s+int|\w+)\s*(?P<rest>.*?)\s*", re.S)
_DECLARATOR = re.compile(r"(?P<stars>(?:\*\s*(?:const\s+)?)*)(?P<name>[A-Za-z_]\w*)?\s*(?P<dims>(?:\[[^\][]*\]\s*)*)")
_OPS = {ast.LShift: int.__lshift__, ast.Add: int.__add__, ast.Sub: int.__sub__, ast.Mult: int.__mul__, ast.BitOr: int.__or__}


class HeaderError(ValueError):
    pass


def _fail(h, at, what):
    """``at``: offset into the text; the line named is that of the first non-blank character from there"""
    at += len(h.text[at:]) - len(h.text[at:].lstrip())
    raise HeaderError(f"line {h.text.count(chr(10), 0, at) + 1}: {what}")


def _int_expr(expr, h, at):
    """an integer constant expression of literals, earlier constants, + - * << | and parentheses"""
    def ev(n):
        if isinstance(n, ast.Constant) and type(n.value) is int:
            return n.value
        if isinstance(n, ast.Name) and n.id in h.constants:
            return h.constants[n.id]
        if isinstance(n, ast.BinOp) and type(n.op) in _OPS:
            return _OPS[type(n.op)](ev(n.left), ev(n.right))
        if isinstance(n, ast.UnaryOp) and isinstance(n.op, ast.USub):
            return -ev(n.operand)
        raise ValueError
    try:
        return ev(ast.parse(expr.strip(), mode="eval").body)
    except (SyntaxError, ValueError, RecursionError):
        _fail(h, at, f"not an integer constant expression: {expr.strip()!r}")


def _declare(decl, h, at, what):
    """``[const] type d1, d2`` -> ("const " or "", type, [(number of *, name or None, [array lengths]), ...])"""
    m = _DECL.fullmatch(decl)
    parts = [_DECLARATOR.fullmatch(d.strip()) for d in m["rest"].split(",")] if m else [None]
    if not all(parts):   # a bit-field, a function pointer, an initialiser, two type words, ...
        _fail(h, at, f"cannot read the {what} {' '.join(decl.split())!r}")
    base = re.sub(r"\s+", " ", m["type"])
    out = [(d["stars"].count("*"), d["name"], [_int_expr(n, h, at) for n in re.findall(r"\[([^\]]*)\]", d["dims"])]) for d in parts]
    for stars, _, dims in out:
        if not (base in SCALARS or base in h.structs or ((stars or dims) and (base == "void" or base in h.opaque))):
            _fail(h, at, f"unknown type {base!r} of the {what} {' '.join(decl.split())!r}")
    return "const " if m["const"] else "", base, out


def _param(decl, h, at, fn):
    """one parameter (or the return type): a scalar, or a pointer -- to a struct of the header POINTER(struct), ``const char *``
    c_char_p, ``const char **`` POINTER(c_char_p), any other c_void_p; an array parameter is a pointer"""
    const, base, names = _declare(decl, h, at, f"parameter of {fn}")
    stars, name, dims = names[0]
    depth = stars + len(dims)
    if len(names) != 1 or len(dims) > 1 or (depth == 0 and base not in SCALARS):
        _fail(h, at, f"{fn}: a parameter is a scalar or a pointer, not {' '.join(decl.split())!r}")
    if depth == 0:
        ctype = SCALARS[base]
    elif base == "char" and depth <= 2:
        ctype = C.c_char_p if depth == 1 else C.POINTER(C.c_char_p)
    else:
        ctype = C.POINTER(h.structs[base]) if base in h.structs and depth == 1 else C.c_void_p
    return Param(name, ctype, f"{const}{base} {'*' * depth}".strip(), depth, base if depth else None)


def _enum(body, h, at):
    nxt = 0
    for item in filter(str.strip, body.split(",")):
        m = re.fullmatch(r"\s*([A-Za-z_]\w*)\s*(?:=(.*))?", item, re.S)
        if not m:
            _fail(h, at, f"cannot read the enumerator {item.strip()!r}")
        h.constants[m[1]] = nxt = _int_expr(m[2], h, at) if m[2] is not None else nxt
        nxt += 1


def _struct(name, body, h, at):
    fields = []
    for m in re.finditer(r"([^;]*);", body):
        _, base, names = _declare(m[1], h, at + m.start(1), "field")
        for stars, fname, dims in names:
            if fname is None:
                _fail(h, at + m.start(1), f"field without a name: {m[1].strip()!r}")
            ctype = C.c_void_p if stars else SCALARS.get(base) or h.structs[base]   # a pointer of any kind: an address
            for n in reversed(dims):
                ctype = ctype * n
            fields.append((fname, ctype))
    if body[body.rfind(";") + 1:].strip():
        _fail(h, at + body.rfind(";") + 1, f"struct {name}: text after the last field")
    return type(name, (C.Structure,), {"_fields_": fields})


def _prototype(stmt, h, at):
    m = re.fullmatch(r"(?P<ret>[\w\s]+?[\s*]+)(?P<name>[A-Za-z_]\w*)\s*\((?P<params>[^()]*)\)\s*", stmt, re.S)
    if not m:
        _fail(h, at, f"cannot read the declaration {' '.join(stmt.split())[:80]!r}")
    ret = Param(None, None, "void", 0, None) if m["ret"].strip() == "void" else _param(m["ret"], h, at, m["name"])
    params = [_param(p[0], h, at + m.start("params") + p.start(), m["name"])
              for p in re.finditer(r"[^,]+", m["params"] if m["params"].strip() != "void" else "")]
    if any(p.name is None for p in params):
        _fail(h, at, f"{m['name']}: a parameter without a name")
    return Proto(m["name"], ret.ctype, ret.ctext, tuple(params))


def parse(text):
    # comments become blanks (newlines kept, so that offsets still tell the line)
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m[0]), text, flags=re.S)
    h = Header({}, {}, {}, set(), text)
    # preprocessor lines: the guard, #include, the __cplusplus block (skipped whole) and #define NAME <integer>
    skip = False
    for m in re.finditer(r"^.*$", text, re.M):
        s = m[0].strip()
        if not (skip or s.startswith("#")):
            continue
        text = text[:m.start()] + " " * len(m[0]) + text[m.end():]
        if skip:
            skip = s != "#endif"
        elif s == "#ifdef __cplusplus":
            skip = True
        elif (d := re.fullmatch(r"#define\s+([A-Za-z_]\w*)\s+(\S.*)", s)):
            h.constants[d[1]] = _int_expr(d[2], h, m.start())
        elif not re.fullmatch(r"#(ifndef\s+\w+|define\s+\w+|endif|include\s+<\w+\.h>)", s):
            _fail(h, m.start(), f"cannot read the preprocessor line {s!r}")
    # statements: up to a ';' outside braces
    start = depth = 0
    for j, ch in enumerate(text):
        depth += (ch == "{") - (ch == "}")
        if ch != ";" or depth:
            continue
        stmt, at = text[start:j].lstrip(), j - len(text[start:j].lstrip())
        start = j + 1
        if (m := re.fullmatch(r"typedef\s+struct\s+(\w+)\s+(\w+)\s*", stmt)):
            h.opaque.add(m[2])
        elif (m := re.fullmatch(r"(?:typedef\s+)?enum\s*\{(.*)\}\s*(\w*)\s*", stmt, re.S)):
            _enum(m[1], h, at)
        elif (m := re.fullmatch(r"typedef\s+struct\s*(\w*)\s*\{(.*)\}\s*(\w+)\s*", stmt, re.S)):
            h.structs[m[3]] = _struct(m[3], m[2], h, at + m.start(2))
        else:
            proto = _prototype(stmt, h, at)
            h.prototypes[proto.name] = proto
    if text[start:].strip() or depth:
        _fail(h, start, "text after the last declaration")
    return h
