"""CPU: argument checks of the frame-interpolation entry points (include/ofdis.h: ofdis_interpolate, ofdis_batch_interpolate)
that return before any device work.  Host buffers stand in for the device arrays: every call here returns before it would
launch.  The computations, and the checks that need a context (creating one needs a device): tests/test_gpu_interp.py."""
import math

import numpy as np
import pytest

import abi
from of_dis_amd import capi


def test_max_times_matches_the_header():
    assert abi.define("OFDIS_INTERP_MAX_TIMES") == capi.INTERP_MAX_TIMES


class _Host:
    """host stand-ins for a 1-frame 8x4 gray case"""

    def __init__(self, w=8, h=4, n=1, noc=1):
        self.img = np.zeros((n, h, w, noc), np.uint8)
        self.flow = np.zeros((n, h, w, 2), np.float32)
        self.mask = np.zeros((n, h, w), np.uint8)
        self.out = np.zeros((n, capi.INTERP_MAX_TIMES, h, w, noc), np.uint8)


def _times(vals):
    t = np.asarray(vals, np.float32)
    return t, t.ctypes.data_as(capi.FP)


def _interp(hb, img_a=True, img_b=True, fw=True, rev=True, out=True, n=1, w=8, h=4, noc=1, times=(0.5,), ntimes=None,
            times_null=False):
    t, tp = _times(times)
    p = abi.ptr
    return capi.lib().ofdis_interpolate(p(hb.img, img_a), p(hb.img, img_b), p(hb.flow, fw), p(hb.flow, rev), hb.mask.ctypes.data,
                                        hb.mask.ctypes.data, p(hb.out, out), n, w, h, noc, None if times_null else tp,
                                        t.size if ntimes is None else ntimes, None)


@pytest.mark.parametrize("which", ["img_a", "img_b", "fw", "rev", "out"])
def test_interpolate_rejects_null_pointers(which):
    assert _interp(_Host(), **{which: False}) == capi.ERR_INVALID
    assert capi.lib().ofdis_last_error()


def test_interpolate_rejects_null_times():
    assert _interp(_Host(), times_null=True) == capi.ERR_INVALID


@pytest.mark.parametrize("ntimes", [0, -1, 17])
def test_interpolate_rejects_ntimes(ntimes):
    assert _interp(_Host(), times=[0.5] * 17, ntimes=ntimes) == capi.ERR_INVALID


BAD_TIMES = [math.nan, math.inf, -math.inf, -1e-7, 1.0000001, 2.0, -1.0]


@pytest.mark.parametrize("bad", BAD_TIMES)
def test_interpolate_rejects_bad_times(bad):
    assert _interp(_Host(), times=[0.5, bad]) == capi.ERR_INVALID
    assert "time" in capi.lib().ofdis_last_error().decode()


@pytest.mark.parametrize("noc", [0, 2, 4, -1])
def test_interpolate_rejects_noc(noc):
    assert _interp(_Host(noc=3), noc=noc) == capi.ERR_INVALID


@pytest.mark.parametrize("n,w,h", [(0, 8, 4), (1, 0, 4), (1, 8, 0), (-1, 8, 4), (1, 1 << 16, 1 << 16), (1, -8, 4)])
def test_interpolate_rejects_bad_sizes(n, w, h):
    assert _interp(_Host(), n=n, w=w, h=h) == capi.ERR_INVALID


def test_interpolate_time_check_accepts_the_closed_unit_interval():
    """every time of [0, 1], both ends and -0.0 included, passes the time check: the call gets as far as the size check"""
    for t in (0.0, -0.0, 1.0, 0.5, 1e-30):
        assert _interp(_Host(), times=[t], n=0) == capi.ERR_INVALID
        assert "size" in capi.lib().ofdis_last_error().decode()


# ------------------------------------------------------------------ ofdis_batch_interpolate
def _batch_call(h, hb, first=0, count=1, times=(0.5,), ntimes=None, img=True, out=True, wo=256, ho=112, alpha=capi.FB_ALPHA,
                beta=capi.FB_BETA, times_null=False):
    t, tp = _times(times)
    return capi.lib().ofdis_batch_interpolate(h, hb.img.ctypes.data if img else None, hb.img.ctypes.data, first, count,
                                              None if times_null else tp, t.size if ntimes is None else ntimes,
                                              hb.out.ctypes.data if out else None, wo, ho, alpha, beta, None)


def test_batch_interpolate_without_a_context():
    assert _batch_call(None, _Host()) == capi.ERR_INVALID
