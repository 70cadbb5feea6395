"""The public headers (include/*.h) as the tests read them: the names they declare and their prototypes taken apart."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("qnnpack.h", "qnnpack_gfx950.h", "qnnpack_gfx950_test.h")

# `ret name(params);` after a statement end or a brace
_PROTOTYPE = re.compile(r"(?:^|[;{}])\s*([^;{}()]+?)\s*\b(qnnp_[a-z0-9_]+)\s*\(([^()]*)\)\s*(?=;)")
_PARAMETER = re.compile(r"(.*?)(\w+)\s*(\[\d*\])?")


def code(header):
    """The header's text without comments and preprocessor lines."""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)


def declared_functions(header):
    return sorted(set(re.findall(r"\b(qnnp_[a-z0-9_]+)\s*\(", code(header))))


def _c_type(text):
    """`const uint8_t *` -> `uint8_t*`: no qualifiers, no blanks around the stars"""
    text = re.sub(r"\bconst\b", "", text)
    return re.sub(r"\s*\*\s*", "*", " ".join(text.split()))


def prototypes(header):
    """{name: (return type, [(parameter type, parameter name), ...])}; an array parameter's type ends in `[]`."""
    found = {}
    for ret, name, params in _PROTOTYPE.findall(code(header)):
        assert name not in found, name
        parsed = []
        if params.strip() != "void":
            for param in params.split(","):
                ctype, pname, array = _PARAMETER.fullmatch(param.strip()).groups()
                parsed.append((_c_type(ctype) + ("[]" if array else ""), pname))
        found[name] = (_c_type(ret), parsed)
    return found
