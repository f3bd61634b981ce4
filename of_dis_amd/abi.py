"""include/ofdis.h read as data: the one parser behind the library's export list (build.py) and the ctypes prototypes of the
binding (capi.py); the tests bind their own library from its header the same way (tests/common.py).  Imports nothing of this
package."""
import ctypes as C
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ofdis.h")

_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_RETURNS = {"int": C.c_int, "size_t": C.c_size_t}  # by value, beside void and the pointers
# What a caller asks for by name (prototypes(text, hook_types=True)): the types the test library's hooks pass and return beside
# the ones above (tests/csrc/ofdis_test_hooks.h).  include/ofdis.h has none of them and is parsed without.
_HOOK_SCALARS = {"long long": C.c_longlong}
_HOOK_RETURNS = {"float": C.c_float, "unsigned": C.c_uint, "long long": C.c_longlong}
_PROTOTYPE = re.compile(r"([A-Za-z_][\w \t*]*?)\s*\b(ofdis_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def _argtype(name, arg, scalars):
    if "*" in arg:  # every pointer, whatever it points to: c_void_p takes byref(), arrays, typed pointers, addresses and None
        return C.c_void_p
    words = arg.split()
    if len(words) < 2 or " ".join(words[:-1]) not in scalars:
        raise ValueError(f"include/ofdis.h: {name}: argument `{arg.strip()}` has a type the binding does not know")
    return scalars[" ".join(words[:-1])]


def _restype(name, ret, returns):
    ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
    if ret == "void":
        return None
    if ret == "const char*":
        return C.c_char_p
    if "*" in ret:
        return C.c_void_p
    if ret in returns:
        return returns[ret]
    raise ValueError(f"include/ofdis.h: {name}: return type `{ret}` is one the binding does not know")


def prototypes(text=None, hook_types=False):
    """name -> (restype, [argtypes]) as ctypes types for every function the header declares, in header order.  A type outside
    the small closed set above raises: a new one in the header is a decision, not a guess.  hook_types: also `long long` by
    value and `float`, `unsigned` and `long long` returns, for the header of the test library."""
    if text is None:
        text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    scalars = {**_SCALARS, **_HOOK_SCALARS} if hook_types else _SCALARS
    returns = {**_RETURNS, **_HOOK_RETURNS} if hook_types else _RETURNS
    out = {}
    for ret, name, args in _PROTOTYPE.findall(text):
        args = args.strip()
        out[name] = (_restype(name, ret, returns),
                     [] if args in ("", "void") else [_argtype(name, a, scalars) for a in args.split(",")])
    return out


def bind(library, protos):
    """Give every function of `protos` (what prototypes returns) its restype and argtypes on a loaded ctypes library, and return
    the library.  A function the library does not export raises AttributeError."""
    for name, (restype, argtypes) in protos.items():
        fn = getattr(library, name)
        fn.restype, fn.argtypes = restype, argtypes
    return library
