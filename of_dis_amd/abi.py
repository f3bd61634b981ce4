"""include/ofdis.h read as data: the one parser behind the library's export list (build.py) and the ctypes prototypes of the
binding (capi.py).  Imports nothing of this package."""
import ctypes as C
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ofdis.h")

_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_PROTOTYPE = re.compile(r"([A-Za-z_][\w \t*]*?)\s*\b(ofdis_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def _argtype(name, arg):
    if "*" in arg:  # every pointer, whatever it points to: c_void_p takes byref(), arrays, typed pointers, addresses and None
        return C.c_void_p
    words = arg.split()
    if len(words) != 2 or words[0] not in _SCALARS:
        raise ValueError(f"include/ofdis.h: {name}: argument `{arg.strip()}` has a type the binding does not know")
    return _SCALARS[words[0]]


def _restype(name, ret):
    ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
    if ret == "void":
        return None
    if ret == "const char*":
        return C.c_char_p
    if "*" in ret:
        return C.c_void_p
    if ret in ("int", "size_t"):
        return _SCALARS[ret]
    raise ValueError(f"include/ofdis.h: {name}: return type `{ret}` is one the binding does not know")


def prototypes(text=None):
    """name -> (restype, [argtypes]) as ctypes types for every function the header declares, in header order.  A type outside
    the small closed set above raises: a new one in the header is a decision, not a guess."""
    if text is None:
        text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for ret, name, args in _PROTOTYPE.findall(text):
        args = args.strip()
        out[name] = (_restype(name, ret), [] if args in ("", "void") else [_argtype(name, a) for a in args.split(",")])
    return out
