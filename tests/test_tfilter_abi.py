"""CPU: the temporal-filter entry points (include/ofdis.h: ofdis_temporal_filter, ofdis_batch_temporal_filter) in the header, the
binding and the export list, and their argument checks that return before any device work.  Host buffers stand in for the device
arrays: every call here returns before it would launch.  The kernels, and the checks that need a context (creating one needs a
device): tests/test_gpu_tfilter.py."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from of_dis_amd import build, capi, temporal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
_f32 = np.float32
FLT_MIN = float(np.finfo(_f32).tiny)
SYMBOLS = ["ofdis_temporal_filter", "ofdis_batch_temporal_filter"]


def _header():
    return open(os.path.join(ROOT, "include", "ofdis.h")).read()


@pytest.mark.parametrize("name", SYMBOLS)
def test_declared_bound_and_exported(name):
    assert name in build.abi_symbols()                      # a declaration outside the header's comments
    assert name in capi.ABI_SYMBOLS
    fn = getattr(capi.lib(), name)
    assert fn.argtypes is not None
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert name in [line.split()[-1] for line in out.splitlines() if line.strip()]


def test_prototypes_match_the_header():
    """the binding's argument lists against the header's declarations, type by type"""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    ctype = {"float": capi.C.c_float, "int": capi.C.c_int}
    for name in SYMBOLS:
        args = re.search(r"\bint " + name + r"\s*\((.*?)\)\s*;", src, re.S).group(1).split(",")
        want = [capi.VP if "*" in a else ctype[a.split()[0]] for a in args]
        assert getattr(capi.lib(), name).argtypes == want, name


def test_the_version_stays():
    assert int(re.search(r"#define OFDIS_VERSION (\d+)", _header()).group(1)) == capi.OFDIS_VERSION == 3


def test_defaults_match_the_binding():
    assert temporal.FB_CONSISTENT == capi.FB_CONSISTENT
    assert (temporal.SUPPORT_PREV, temporal.SUPPORT_NEXT) == (1, 2)


def test_the_header_states_the_two_consequences():
    hdr = _header()
    section = hdr[hdr.index("Motion-compensated temporal filtering"):hdr.index("int ofdis_batch_temporal_filter")]
    assert "wn = 0 returns the clip bit for bit" in section
    assert re.search(r"identical frames with zero flows returns\s+\*?\s*itself", section)


class _Host:
    """host stand-ins for a 2-pair 8x4 case"""

    def __init__(self, w=8, h=4, npairs=2, noc=1):
        self.frames = np.zeros((npairs + 1, h, w, noc), np.uint8)
        self.flow = np.zeros((npairs, h, w, 2), _f32)
        self.mask = np.zeros((npairs, h, w), np.uint8)
        self.out = np.zeros((npairs + 1, h, w, noc), np.uint8)
        self.support = np.zeros((npairs + 1, h, w), np.uint8)


def _filter(hb, frames=True, fw=True, rev=True, out=True, in_place=False, npairs=2, w=8, h=4, noc=1, wn=1.0, tau=math.inf):
    p = lambda a, on: a.ctypes.data if on else None
    return capi.lib().ofdis_temporal_filter(p(hb.frames, frames), p(hb.flow, fw), p(hb.flow, rev), hb.mask.ctypes.data,
                                            hb.mask.ctypes.data, p(hb.frames, True) if in_place else p(hb.out, out),
                                            hb.support.ctypes.data, npairs, w, h, noc, wn, tau, None)


def _rejected(rc, word=None):
    assert rc == INVALID
    msg = capi.lib().ofdis_last_error().decode()
    assert msg and (word is None or word in msg), msg


@pytest.mark.parametrize("which", ["frames", "fw", "rev", "out"])
def test_temporal_filter_rejects_null_pointers(which):
    _rejected(_filter(_Host(), **{which: False}))


def test_temporal_filter_rejects_in_place():
    _rejected(_filter(_Host(), in_place=True), "in place")


@pytest.mark.parametrize("noc", [0, 2, 4, -1])
def test_temporal_filter_rejects_noc(noc):
    _rejected(_filter(_Host(noc=3), noc=noc), "noc")


@pytest.mark.parametrize("npairs,w,h", [(0, 8, 4), (-1, 8, 4), (2, 0, 4), (2, 8, 0), (2, -8, 4), (2, 1 << 16, 1 << 16)])
def test_temporal_filter_rejects_bad_sizes(npairs, w, h):
    _rejected(_filter(_Host(), npairs=npairs, w=w, h=h), "size")


@pytest.mark.parametrize("wn", [-1e-7, 1.0000001, 2.0, -1.0, math.nan, math.inf, -math.inf])
def test_temporal_filter_rejects_wn(wn):
    _rejected(_filter(_Host(), wn=wn), "wn")


@pytest.mark.parametrize("tau", [0.0, -0.0, -1.0, -math.inf, math.nan, FLT_MIN / 2, 1e-45])
def test_temporal_filter_rejects_tau(tau):
    _rejected(_filter(_Host(), tau=tau), "tau")


def test_the_value_checks_accept_their_closed_ranges():
    """both ends of [0, 1] and -0.0 for wn; +inf, FLT_MIN and FLT_MAX for tau: the call gets as far as the size check"""
    for wn in (0.0, -0.0, 1.0, 0.5, 1e-30):
        _rejected(_filter(_Host(), wn=wn, npairs=0), "size")
    for tau in (math.inf, FLT_MIN, float(np.finfo(_f32).max), 1.5):
        _rejected(_filter(_Host(), tau=tau, npairs=0), "size")


def test_batch_temporal_filter_without_a_context():
    hb = _Host()
    rc = capi.lib().ofdis_batch_temporal_filter(None, hb.frames.ctypes.data, 0, 2, hb.out.ctypes.data, None, 8, 4, 1.0, math.inf,
                                                capi.FB_ALPHA, capi.FB_BETA, None)
    _rejected(rc)
