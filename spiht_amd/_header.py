"""include/spiht_hip.h read as the ctypes binding: prototypes, structs and enumerators.

The whole mapping.  By value: int, int32_t, uint32_t, int64_t, uint64_t, uint8_t and double, to the ctypes scalar of that width
and signedness.  `const char *`: c_char_p, as an argument and as a result.  Every other pointer: c_void_p -- the header cannot
tell an array on the device from one value the call fills, and c_void_p takes what callers pass: integers, None, byref(),
pointer(), ctypes arrays.  A result is int, `const char *` or void.  Anything else is an error that names the declaration.
"""
import ctypes as C
import re

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "uint8_t": C.c_uint8, "double": C.c_double}


def ctype(decl, where):
    """the ctypes type of `type` or `type name`, as the parameter, field or result `where`"""
    words = re.sub(r"\bconst\b", " ", decl).replace("*", " * ").split()
    if "*" in words:
        return C.c_char_p if words[:2] == ["char", "*"] and words.count("*") == 1 else C.c_void_p
    if len(words) > 2 or not words or words[0] not in SCALARS:
        raise ValueError("%s: no ctypes mapping for '%s'" % (where, " ".join(decl.split())))
    return SCALARS[words[0]]


def parse(text):
    """the header's text -> (functions {name: (restype, [argtypes])} in the header's order,
    structs {name: [(field, type)]}, enumerators {name: value})"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)   # (no macro of the header runs over a line)
    text = re.sub(r'\bextern\s+"C"\s*\{', " ", text)
    enums, structs, functions = {}, {}, {}

    def enum(m):
        value = -1
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            name, _, v = (s.strip() for s in item.partition("="))
            enums[name] = value = int(v, 0) if v else value + 1
        return " "

    def struct(m):
        fields = structs[m.group(2)] = []
        for stmt in filter(None, (s.strip() for s in m.group(1).split(";"))):
            first, *more = (s.strip() for s in stmt.split(","))   # `int64_t sc, sh, sw`
            base = re.sub(r"[\s*]*\w+$", "", first)
            for d in [first] + [base + " " + s for s in more]:
                name = re.search(r"\w+$", d).group()
                fields.append((name, ctype(d, "%s.%s" % (m.group(2), name))))
        return " "

    text = re.sub(r"\benum\s*\w*\s*\{([^}]*)\}\s*;", enum, text)
    text = re.sub(r"\btypedef\s+struct\s+\w+\s*\{([^}]*)\}\s*(\w+)\s*;", struct, text)
    for stmt in text.split(";"):
        if "(" not in stmt:   # `typedef struct spiht_ctx spiht_ctx`, the closing brace of extern "C"
            continue
        m = re.fullmatch(r"\s*([\w\s*]+?)\b(\w+)\s*\(([^()]*)\)\s*", stmt)
        if not m:
            raise ValueError("not a prototype: '%s'" % " ".join(stmt.split()))
        ret, name, params = m.groups()
        params = [] if params.strip() == "void" else params.split(",")
        functions[name] = (None if ret.split() == ["void"] else ctype(ret + " _", name + "()"),
                           [ctype(p, "%s(), parameter %d" % (name, i + 1)) for i, p in enumerate(params)])
    return functions, structs, enums
