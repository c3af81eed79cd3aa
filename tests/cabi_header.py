"""The one reader of include/rotmvgaze.h on the Python side: every test that asks what the C ABI declares asks here.

Parsed once at import:
  functions  name -> (return C type, [(C type, parameter name), ...])
  structs    name -> [(field name, C base type, array length or None), ...]; None for an opaque forward declaration
  constants  name -> int, for every `#define MVG_X <int>` and every enumerator with an explicit value
  text       the header as written, for a test that pins a sentence of its prose
A C type is written without `const` and without spaces around its stars: "int64_t", "float*", "void**", "mvg_session**".
Anything the parser cannot classify raises HeaderError: no declaration is ever skipped.
"""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rotmvgaze.h")

SCALARS = ("int", "int32_t", "int64_t", "size_t", "float", "double", "uint8_t", "uint16_t", "uint32_t", "uint64_t")
GUARD = "ROTMVGAZE_H"                            # the include guard
_ID = r"[A-Za-z_]\w*"
_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"


class HeaderError(Exception):
    pass


def _preprocess(text, constants):
    """Drop comments; take `#define NAME <int>` into `constants`; keep only what a C compiler (no __cplusplus) sees."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    if "/*" in text or "*/" in text or "//" in text:
        raise HeaderError("unterminated or line comment")
    out, live = [], [True]                       # `live`: one entry per open #if, True while its lines count
    for line in text.split("\n"):
        s = line.strip()
        if not s.startswith("#"):
            if all(live):
                out.append(line)
            continue
        if s.endswith("\\"):
            raise HeaderError(f"continued preprocessor line: {s}")
        d = s[1:].split()
        if d == ["ifdef", "__cplusplus"]:
            live.append(False)                   # the extern "C" wrapper
        elif d == ["ifndef", GUARD]:
            live.append(True)
        elif d[0] == "endif" and len(live) > 1:
            live.pop()
        elif not all(live):
            continue
        elif d[0] == "include" and len(d) == 2:
            continue
        elif d == ["define", GUARD]:
            continue
        elif d[0] == "define" and len(d) == 3 and re.fullmatch(_ID, d[1]) and re.fullmatch(_INT, d[2]):
            _put(constants, d[1], int(d[2], 0))
        else:
            raise HeaderError(f"preprocessor line not understood: {s}")
    if len(live) != 1:
        raise HeaderError("unbalanced #if / #endif")
    return "\n".join(out)


def _put(table, name, value):
    if name in table:
        raise HeaderError(f"{name} declared twice")
    table[name] = value


def _statements(text):
    """Top-level declarations: the text between semicolons outside braces."""
    depth, start = 0, 0
    for i, ch in enumerate(text):
        if ch == "{":
            depth += 1
        elif ch == "}":
            depth -= 1
            if depth < 0:
                raise HeaderError("unbalanced braces")
        elif ch == ";" and depth == 0:
            s = " ".join(text[start:i].split())
            if not s:
                raise HeaderError("empty declaration")
            yield s
            start = i + 1
    if depth or text[start:].strip():
        raise HeaderError(f"text after the last declaration: {text[start:].strip()[:60]!r}")


def _ctype(text, known):
    """'const float *const *' -> 'float**'; the base must be a scalar, void, char or a struct declared so far."""
    words = [w for w in text.replace("*", " * ").split() if w != "const"]
    base, stars = [w for w in words if w != "*"], words.count("*")
    if len(base) != 1 or words[:1] != base or base[0] not in known:
        raise HeaderError(f"type not understood: {text!r}")
    return base[0] + "*" * stars


def _parameter(text, known):
    m = re.fullmatch(r"(.*[\s*])(%s)" % _ID, text.strip())
    if not m:
        raise HeaderError(f"parameter not understood: {text!r}")
    return _ctype(m.group(1), known), m.group(2)


def _fields(body):
    out = []
    decls = body.split(";")
    if decls.pop().strip():
        raise HeaderError(f"struct field without a semicolon: {body!r}")
    for decl in decls:
        m = re.fullmatch(r"\s*(%s)\s+(.*)" % _ID, decl, flags=re.S)
        if not m or m.group(1) not in SCALARS:
            raise HeaderError(f"struct field not understood: {decl.strip()!r}")
        for item in m.group(2).split(","):
            f = re.fullmatch(r"\s*(%s)\s*(?:\[\s*(\d+)\s*\])?\s*" % _ID, item)
            if not f:
                raise HeaderError(f"struct field not understood: {decl.strip()!r}")
            out.append((f.group(1), m.group(1), int(f.group(2)) if f.group(2) else None))
    if len({n for n, _, _ in out}) != len(out):
        raise HeaderError(f"struct field named twice: {body!r}")
    return out


def parse(text):
    functions, structs, constants = {}, {}, {}
    known = lambda: set(SCALARS) | {"void", "char"} | set(structs)
    for s in _statements(_preprocess(text, constants)):
        m = re.fullmatch(r"enum \{(.*)\}", s)
        if m:
            for item in m.group(1).split(","):
                e = re.fullmatch(r"\s*(%s)\s*=\s*(%s)\s*" % (_ID, _INT), item)
                if not e:
                    raise HeaderError(f"enumerator without an explicit integer value: {item.strip()!r}")
                _put(constants, e.group(1), int(e.group(2), 0))
            continue
        m = re.fullmatch(r"typedef struct (%s) (%s)" % (_ID, _ID), s)
        if m and m.group(1) == m.group(2):
            _put(structs, m.group(1), None)
            continue
        m = re.fullmatch(r"typedef struct (?:(%s) )?\{(.*)\} (%s)" % (_ID, _ID), s)
        if m and m.group(1) in (None, m.group(3)):
            _put(structs, m.group(3), _fields(m.group(2)))
            continue
        m = re.fullmatch(r"([^(){}]*[\s*])(%s) ?\(([^(){}]*)\)" % _ID, s)
        if m:
            params = m.group(3).strip()
            args = [] if params == "void" else [_parameter(p, known()) for p in params.split(",")]
            if len({n for _, n in args}) != len(args):
                raise HeaderError(f"{m.group(2)}: parameter named twice")
            _put(functions, m.group(2), (_ctype(m.group(1), known()), args))
            continue
        raise HeaderError(f"declaration not understood: {s[:100]!r}")
    return functions, structs, constants


with open(HEADER) as _f:
    text = _f.read()                             # for the few tests that pin a sentence of the header's prose
functions, structs, constants = parse(text)


def arity(name):
    return len(functions[name][1])


def parameter_names(name):
    return [n for _, n in functions[name][1]]


def field_names(struct):
    return [n for n, _, _ in structs[struct]]
