"""Reader of include/vampire_hip.h: the header is the one statement of the C ABI, and this module turns it into plain
data for the ctypes binding (_capi.py) and for the tests.

It understands exactly what that header is written in -- `#define NAME integer`, anonymous enums, `typedef struct`
with scalar, pointer, nested-structure and array fields, and function prototypes -- and raises HeaderError, naming the
line, on anything else: a declaration it skipped would be a symbol found missing on the GPU.
"""
import os
import re
import typing

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vampire_hip.h")

SCALARS = ("void", "char", "int", "float", "double", "size_t", "int8_t", "int16_t", "int32_t", "int64_t", "uint8_t",
           "uint32_t", "uint64_t")


class HeaderError(ValueError):
    pass


class Header(typing.NamedTuple):
    constants: dict      # {name: int}, the #defines and enumerators in header order
    structs: dict        # {name: [(field, C type, dims)]}, dims a tuple of ints (() for a plain field)
    prototypes: dict     # {name: (return type, [(C type, parameter name)])}; an array parameter is a pointer


_IGNORED = re.compile(r'#\s*(?:ifndef|ifdef|endif|include)\b.*|#\s*define\s+\w+_H_|extern\s+"C"\s*\{|\}')
_SPACE = re.compile(r"\s*")
_DEFINE = re.compile(r"#\s*define\s+(\w+)[ \t]+(.+)")
_ENUM = re.compile(r"enum\s*\{([^{};]*)\}\s*;")
_STRUCT = re.compile(r"typedef\s+struct\s*(\w*)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO = re.compile(r"([\w\s*]+?)(\w+)\s*\(([^(){};]*)\)\s*;")
_DECLARATOR = re.compile(r"(.*?)(\w+)\s*((?:\[\s*\w*\s*\]\s*)*)$", re.S)


def parse(text) -> Header:
    # comments become blanks of the same height, so that a position still says its line
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group().count("\n") or " ", text, flags=re.S)
    constants, structs, prototypes = {}, {}, {}

    def fail(pos, what):
        raise HeaderError(f"line {text.count(chr(10), 0, pos) + 1}: {what}")

    def value(expr, pos):
        expr = expr.strip()
        if expr.startswith("(") and expr.endswith(")"):
            expr = expr[1:-1].strip()
        if expr in constants:
            return constants[expr]
        try:
            return int(expr, 0)
        except ValueError:
            fail(pos, f"cannot evaluate {expr!r}")

    def ctype(spelling, pos):
        """`const  float *` -> `const float*`, after checking that it names a type this header may use."""
        spelling = " ".join(spelling.split()).replace(" *", "*")
        base = re.sub(r"\bconst\b|\*", " ", spelling).split()
        if len(base) != 1 or not (base[0] in SCALARS or base[0] in structs):
            fail(pos, f"unknown type {spelling!r}")
        return spelling

    def declarator(decl, pos):
        m = _DECLARATOR.match(decl.strip())
        if not m:
            fail(pos, f"cannot parse the declaration {decl.strip()!r}")
        return m.group(1), m.group(2), re.findall(r"\[\s*(\w*)\s*\]", m.group(3))

    pos = 0
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            return Header(constants, structs, prototypes)
        if m := _IGNORED.match(text, pos):
            pass
        elif m := _DEFINE.match(text, pos):
            constants[m.group(1)] = value(m.group(2), pos)
        elif m := _ENUM.match(text, pos):
            nxt = 0
            for item in filter(None, (i.strip() for i in m.group(1).split(","))):
                name, _, expr = (s.strip() for s in item.partition("="))
                if not re.fullmatch(r"\w+", name):
                    fail(pos, f"cannot parse the enumerator {item!r}")
                constants[name] = nxt = value(expr, pos) if expr else nxt
                nxt += 1
        elif m := _STRUCT.match(text, pos):
            if m.group(1) not in ("", m.group(3)):
                fail(pos, f"struct {m.group(1)} is given another name, {m.group(3)}")
            fields = []
            for decl in filter(None, (d.strip() for d in m.group(2).split(";"))):
                first, *more = decl.split(",")
                spelling, name, dims = declarator(first, pos)
                kind = ctype(spelling, pos)
                rest = [declarator(d, pos) for d in more]
                if rest and ("*" in kind or any(r[0].strip() for r in rest)):    # (`T* a, b`: b is no pointer in C)
                    fail(pos, f"one pointer field per declaration, please: {decl!r}")
                for n, dm in [(name, dims)] + [r[1:] for r in rest]:
                    fields.append((n, kind, tuple(value(x, pos) for x in dm)))
            structs[m.group(3)] = fields
        elif m := _PROTO.match(text, pos):
            params = []
            if m.group(3).strip() not in ("", "void"):
                for prm in m.group(3).split(","):
                    spelling, name, dims = declarator(prm, pos)
                    params.append((ctype(spelling + "*" * len(dims), pos), name))
            prototypes[m.group(2)] = (ctype(m.group(1), pos), params)
        else:
            fail(pos, f"cannot parse {text[pos:pos + 60].splitlines()[0]!r}")
        pos = m.end()


_parsed = None


def read() -> Header:
    """The project's header, parsed once per process."""
    global _parsed
    if _parsed is None:
        with open(HEADER) as f:
            _parsed = parse(f.read())
    return _parsed
