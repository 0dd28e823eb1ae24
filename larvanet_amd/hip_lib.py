"""ctypes binding of liblarva_hip.so (the C ABI declared in include/larva_hip.h).

The header is the only place an entry point's types are written down: SIGNATURES is parsed from it at import
(parse_header), so a new entry point needs its declaration, its .hip definition and its wrapper in kernels.py, nothing
here.  A declaration the parser cannot type, a missing header and a symbol the library does not export all raise.

There is no fallback: if the library is missing or a call fails, a RuntimeError is raised.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "liblarva_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "larva_hip.h")

_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
            "long long": ctypes.c_longlong}


def _ctype(text, decl, named):
    """One C type of a declaration (`named`: a parameter, whose name is dropped) -> its ctypes type."""
    stars = text.count("*")
    words = re.sub(r"\bconst\b|\*", " ", text).split()
    if named and len(words) > 1:
        words.pop()
    base = " ".join(words)
    if stars:
        # device pointers travel as integers; host arrays, byref() and None pass as c_void_p too
        return ctypes.c_char_p if base == "char" and not named else ctypes.c_void_p
    if base == "void" and not named:
        return None
    if base not in _SCALARS:
        raise RuntimeError("larvanet_amd: no ctypes type for `%s` in the declaration `%s`" % (text.strip(), decl))
    return _SCALARS[base]


def parse_header(path):
    """name -> (restype, [argtypes]) of every `ret larva_name(args);` a C header declares.  Comments, preprocessor lines,
    `typedef struct` blocks and the extern "C" braces are stepped over; anything else raises: nothing is skipped and
    nothing gets a default type."""
    if not os.path.exists(path):
        raise RuntimeError("larvanet_amd: %s is missing: the ctypes binding is derived from it" % path)
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    text = re.sub(r"//[^\n]*|^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r"\btypedef\s+struct\b[^{;]*\{.*?\}[^;]*;", " ", text, flags=re.S)
    text = re.sub(r'\bextern\s+"C"\s*\{|\}', " ", text)
    signatures = {}
    for decl in (" ".join(d.split()) for d in text.split(";")):
        if not decl:
            continue
        m = re.fullmatch(r"(.+?)\b(larva_\w+) ?\((.*)\)", decl)
        if m is None or m.group(2) in signatures:
            raise RuntimeError("larvanet_amd: %s: cannot bind `%s`" % (path, decl))
        args = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
        signatures[m.group(2)] = (_ctype(m.group(1), decl, False), [_ctype(a, decl, True) for a in args])
    return signatures


SIGNATURES = parse_header(HEADER_PATH)   # name -> (restype, argtypes)

_lib = None


def load():
    """Load (once) and return the ctypes handle. Raises RuntimeError if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # LARVA_HIP_LIB: another build of the same sources (same-box A/B timing of compile-time options)
    path = os.environ.get("LARVA_HIP_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(
            "larvanet_amd: %s is missing. Build it with `python -m larvanet_amd.build` "
            "(hipcc --offload-arch=gfx950); there is no CPU or PyTorch fallback." % path)
    # torch must own the process's HIP runtime: loading this library first would bring in a
    # second libamdhip64 that later finds "no ROCm-capable device".
    import torch  # noqa: F401
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header and library disagree
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code, what):
    if code != 0:
        lib = load()
        msg = lib.larva_error_string(code)
        raise RuntimeError("larvanet_amd: %s failed: hip error %d (%s)" %
                           (what, code, msg.decode() if msg else "?"))


def ptr_array(ptrs):
    """Array of device pointers (ints / None) for a `const float* const*` argument."""
    arr = (ctypes.c_void_p * len(ptrs))()
    for i, p in enumerate(ptrs):
        arr[i] = p
    return arr


def int_array(vals):
    return (ctypes.c_int * len(vals))(*vals)
