"""CPU: the TEST library (libofdis_testhooks.so) exports exactly the functions tests/csrc/ofdis_test_hooks.h declares, and the
parser that binds them (of_dis_amd/abi.py, with the types only the hooks use) reads that header as written here by hand.

The hook files include the header and define their functions as extern "C", so a definition that disagrees with its
declaration does not compile.  What the compiler cannot see is a definition that is not extern "C" (a C++ overload: the C name
is then missing from the library) and a hook without a declaration (exported, but unbound): both change the symbol set."""
import ctypes as C
import subprocess

import pytest

import common
from of_dis_amd import build
from of_dis_amd.abi import prototypes

PROTOTYPES = common.testhook_prototypes()
I, U, F, LL, Z, P = C.c_int, C.c_uint, C.c_float, C.c_longlong, C.c_size_t, C.c_void_p
UPG = [I] * 7   # UpGeom: sw, sh, sc_l, left, top, wo, ho
# one hook of each shape, written by hand: (restype, argtypes)
EXPECTED = {
    "ofdis_test_launch_interp_bidir": (I, [P] * 5 + [I] + UPG + [I, P, I, F, F, P]),   # pointers and the seven ints of UpGeom
    "ofdis_test_launch_lr_materialise": (I, [P] * 4 + [I] + UPG + [P]),
    "ofdis_test_set_launch_limits": (None, [LL, LL]),                                  # long long by value
    "ofdis_test_xcd_grid": (LL, [I, LL]),                                              # ... and returned
    "ofdis_test_grid_for": (U, [LL]),                                                  # unsigned return
    "ofdis_test_outlier_sq": (F, [F]),                                                 # float return
    "ofdis_test_segments_work_bytes": (Z, [I, I, I]),                                  # size_t return
    "ofdis_test_launch_pyr_base": (I, [P, P] + [I] * 7 + [Z, Z, P]),                   # size_t by value
    "ofdis_test_launch_label_segments": (I, [P, P, I, I, I, U, I, I, I, P, P, P, P, P]),   # unsigned by value
    "ofdis_test_quad_grid": (None, [I, I, I, P, P]),
}


def _exported():
    out = subprocess.run(["nm", "-D", "--defined-only", build.testhooks_path()], capture_output=True, text=True, check=True).stdout
    names = [line.split()[-1] for line in out.splitlines() if line.strip()]
    return sorted(n for n in names if n.startswith("ofdis_test_"))


def test_the_header_declares_what_the_library_exports():
    exported = _exported()
    assert sorted(PROTOTYPES) == exported, sorted(set(PROTOTYPES) ^ set(exported))
    assert len(exported) == 49 and len(set(exported)) == 49


def test_every_declared_hook_is_bound():
    L = common.testhooks()
    assert common.testhooks() is L   # opened once
    import launch_hooks
    assert launch_hooks.hooks() is L
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and (fn.restype, list(fn.argtypes)) == (restype, argtypes), name


@pytest.mark.parametrize("name", EXPECTED)
def test_the_parser_gives_the_hook_prototypes_written_here(name):
    assert PROTOTYPES[name] == EXPECTED[name]


def test_launch_hooks_return_a_status_and_end_in_the_stream():
    launchers = [n for n in PROTOTYPES if n.startswith("ofdis_test_launch_")]
    assert len(launchers) == 29
    for name in launchers:
        ret, args = PROTOTYPES[name]
        assert ret is I and args[-1] is P, name


def test_the_hook_types_are_asked_for_by_name():
    """called as the product's binding calls it, the parser refuses what only the hooks need"""
    for text, word in (("void ofdis_test_a(long long n);", "long long n"), ("float ofdis_test_b(float t);", "float"),
                       ("unsigned ofdis_test_c(int n);", "unsigned"), ("long long ofdis_test_d(int n);", "long long")):
        with pytest.raises(ValueError, match=word):
            prototypes(text)
        assert len(prototypes(text, hook_types=True)) == 1
    with pytest.raises(ValueError, match="short x"):   # and with them, still nothing else
        prototypes("int ofdis_test_e(short x);", hook_types=True)
    with pytest.raises(ValueError, match="ofdis_test_f"):
        prototypes("double ofdis_test_f(void);", hook_types=True)
