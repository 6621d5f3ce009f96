"""The prototypes of libmsfm.so, read from include/msfm.h: every declaration `ret msfm_name(params);` outside a typedef
becomes (restype, argtypes) through one table of type shapes.  What the table does not hold is refused, not guessed."""
import ctypes as C
import os
import re

from . import _abi as A

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "msfm.h")
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)

# a shape: the tokens of a parameter without `const` and without its name; an array parameter (`double F[9]`) is a pointer
SHAPES = {"int": C.c_int, "double": C.c_double, "float": C.c_float, "size_t": C.c_size_t, "uint64_t": C.c_uint64,
          "double *": A.c_double_p, "float *": A.c_float_p, "int *": A.c_int_p, "int32_t *": A.c_int_p,
          "int64_t *": C.POINTER(C.c_int64), "uint8_t *": A.c_u8_p, "uint16_t *": C.POINTER(C.c_uint16),
          "uint32_t *": C.POINTER(C.c_uint32), "unsigned char *": C.POINTER(C.c_ubyte), "void *": C.c_void_p,
          "float * *": C.POINTER(A.c_float_p), "int32_t * *": C.POINTER(A.c_int_p), "msfm_allreduce_fn": ALLREDUCE_FN}
RETURNS = {"int": C.c_int, "void": None, "char *": C.c_char_p, "void *": C.c_void_p, "msfm_ctx *": C.c_void_p}


def strip_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)


def struct_names(text):
    """The structs the header defines (`typedef struct msfm_x { ... } msfm_x;`), in its order."""
    return re.findall(r"typedef\s+struct\s+(msfm_\w+)\s*\{", strip_comments(text))


def mirror(struct_name):
    """The ctypes mirror of a struct of the header, by name: msfm_round_options -> _abi.RoundOptions (None: there is none)."""
    cls = getattr(A, "".join(w.capitalize() for w in struct_name[len("msfm_"):].split("_")), None)
    return cls if isinstance(cls, type) and issubclass(cls, C.Structure) else None


def _shape(decl, named):
    tok = [t for t in re.findall(r"\w+|\*", decl.split("[")[0]) if t != "const"]
    if named and tok[-1:] == ["*"]:      # a parameter without a name: its last token would be taken for one
        return ""
    return " ".join(tok[:len(tok) - named] + ["*"] * ("[" in decl))


def bind(L, protos):
    """The loaded library L with restype / argtypes of every prototype set."""
    for name, (restype, argtypes) in protos.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    return L


def prototypes(text):
    """{name: (restype, argtypes)} of every function the header text declares; ImportError names the declaration it refuses."""
    text = strip_comments(text)
    names = set(re.findall(r"\b(msfm_[a-z0-9_]+)\s*\(", text)) - {"msfm_allreduce_fn"}
    shapes = dict(SHAPES)
    for s in re.findall(r"typedef\s+struct\s+(\w+)\s+\1\s*;", text):                  # the opaque handle types
        shapes[s + " *"], shapes[s + " * *"] = C.c_void_p, C.POINTER(C.c_void_p)
    for s in struct_names(text):
        shapes[s + " *"] = C.POINTER(mirror(s)) if mirror(s) else "struct %s has no mirror in _abi.py" % s
    body = re.sub(r"typedef\b[^;{]*(\{[^}]*\}[^;]*)?;", "", re.sub(r"^\s*#.*$", "", text, flags=re.M))
    out = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(msfm_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", body):
        found = [(ret, RETURNS.get(_shape(ret, 0), "no such return type"))]
        found += [(p, shapes.get(_shape(p, 1), "no such type shape")) for p in params.split(",") if params.strip() != "void"]
        for decl, typ in found:
            if isinstance(typ, str):
                raise ImportError("include/msfm.h, %s: `%s`: %s" % (name, " ".join(decl.split()), typ))
        out[name] = (found[0][1], [typ for _, typ in found[1:]])
    if set(out) != names:
        raise ImportError("include/msfm.h: declarations not understood: %s" % ", ".join(sorted(set(out) ^ names)))
    return out
