"""The C ABI as include/*.h declares it, parsed once at import: the ctypes binding (_lib.py), the descriptor Structures (sd/ops.py,
seg/ops.py) and the constants all come from here, so there is no second copy of a prototype to keep in step.

    FUNCTIONS   name -> (restype, [(parameter name, ctype), ...]), in header order
    STRUCTS     typedef name -> [(field name, ctype), ...]
    DEFINES     NAME -> int: every `#define NAME <integer>` / `#define NAME (-n)` and every enum member

The headers are plain C in one uniform style and parse() reads exactly that style with regular expressions.  It never guesses: a type
outside TYPES, a parameter without a name, an array, function-pointer or variadic parameter, a bit-field, a nested struct, or ANY text
that is not a comment, a preprocessor line, a struct, an enum, a prototype or the `extern "C" { }` pair raises AbiError with the header's
name and the offending text -- a declaration the parser cannot read stops the import instead of vanishing from the binding.

Pointers: `const char*` is c_char_p (returns included), every other pointer is c_void_p -- wrappers pass device addresses as integers,
and c_void_p also takes the ctypes arrays, byref(...) and None that callers pass for host-side parameters.  ctypes therefore does not
check the element type of a host array; that guarantee lives where the arrays are built (_lib.vec3 makes c_float * 3, the parents
tables are made as c_int32 * J)."""
import ctypes as C
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

# every scalar the headers use, by value or behind a pointer
TYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "long long": C.c_longlong, "size_t": C.c_size_t,
         "float": C.c_float, "double": C.c_double, "int8_t": C.c_int8, "uint8_t": C.c_uint8, "uint64_t": C.c_uint64}

_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"


class AbiError(RuntimeError):
    pass


def header_paths():
    return sorted(os.path.join(INCLUDE, f) for f in os.listdir(INCLUDE) if f.endswith(".h"))


def parse(text, header="<string>"):
    """Header text -> (functions, structs, defines) as described above."""
    functions, structs, defines = {}, {}, {}

    def fail(why, what):
        raise AbiError(f"{header}: {why}: {' '.join(what.split())!r}")

    def ctype(spec, what, void=False):
        """ctypes type of a C type written as `spec`; `what` is the declaration it stands in (for the message)"""
        base = " ".join(re.sub(r"\bconst\b|\*", " ", spec).split())
        stars = spec.count("*")
        if stars:
            if base not in TYPES and base not in structs and base not in ("void", "char"):
                fail("type outside the map", what)
            return C.c_char_p if base == "char" and stars == 1 else C.c_void_p
        if base == "void" and void:
            return None
        if base not in TYPES:
            fail("type outside the map", what)
        return TYPES[base]

    def declaration(decl, kind):
        """`type name` (a field: `type name, name`) -> [(name, ctype), ...]"""
        if "..." in decl:
            fail(f"variadic {kind}", decl)
        if "(" in decl:
            fail(f"function-pointer {kind}", decl)
        if "[" in decl:
            fail(f"array {kind}", decl)
        if ":" in decl:
            fail("bit-field", decl)
        m = re.fullmatch(r"(.+?[\s*])(\w+(?:\s*,\s*\w+)*)", decl.strip(), re.S)
        if not m:
            fail(f"{kind} without a name", decl)
        if "*" in m.group(1) and "," in m.group(2):
            fail("several pointers in one declaration", decl)
        t = ctype(m.group(1), decl)
        return [(n, t) for n in re.split(r"\s*,\s*", m.group(2))]

    def add(table, name, value, what):
        if name in table:
            fail("declared twice", what)
        table[name] = value

    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(?:(%s)|\([ \t]*(%s)[ \t]*\))[ \t]*$" % (_INT, _INT), text, re.M):
        add(defines, m.group(1), int(m.group(2) or m.group(3), 0), m.group(0))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)

    def struct(m):
        if "{" in m.group(1) or re.search(r"\b(struct|union)\b", m.group(1)):
            fail("nested struct", m.group(0))
        fields = [f for d in m.group(1).split(";") if d.strip() for f in declaration(d, "field")]
        add(structs, m.group(2), fields, m.group(2))
        return ""

    def enum(m):
        value = -1
        for member in filter(None, (s.strip() for s in m.group(1).split(","))):
            mm = re.fullmatch(r"(\w+)(?:\s*=\s*(%s))?" % _INT, member)
            if not mm:
                fail("enum member", member)
            value = int(mm.group(2), 0) if mm.group(2) else value + 1
            add(defines, mm.group(1), value, member)
        return ""

    text = re.sub(r"\btypedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    text = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, text)
    text = re.sub(r'\bextern\s+"C"\s*\{(.*)\}', r"\1", text, count=1, flags=re.S)
    for stmt in text.split(";"):
        if not stmt.strip():
            continue
        m = re.fullmatch(r"\s*([\w\s*]+?[\s*])((?:coma|sd|seg)_\w+)\s*\((.*)\)\s*", stmt, re.S)
        if not m:
            fail("text that is no declaration this parser reads", stmt)
        params = [] if m.group(3).strip() == "void" else [declaration(p, "parameter")[0] for p in m.group(3).split(",")]
        add(functions, m.group(2), (ctype(m.group(1), stmt, void=True), params), m.group(2))
    return functions, structs, defines


FUNCTIONS, STRUCTS, DEFINES = {}, {}, {}
for _path in header_paths():
    with open(_path) as _f:
        for _table, _found in zip((FUNCTIONS, STRUCTS, DEFINES), parse(_f.read(), os.path.basename(_path))):
            _twice = sorted(set(_table) & set(_found))
            if _twice:
                raise AbiError(f"{os.path.basename(_path)}: declared in an earlier header too: {_twice}")
            _table.update(_found)
