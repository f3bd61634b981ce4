"""CPU: the temporal-filter entry points (include/ofdis.h: ofdis_temporal_filter, ofdis_batch_temporal_filter) in the header, the
binding and the export list, and their argument checks that return before any device work.  Host buffers stand in for the device
arrays: every call here returns before it would launch.  The kernels, and the checks that need a context (creating one needs a
device): tests/test_gpu_tfilter.py."""
import math
import re

import numpy as np
import pytest

import abi
from of_dis_amd import capi, temporal
from seq_products import FLT_MIN

_f32 = np.float32


def test_defaults_match_the_binding():
    assert temporal.FB_CONSISTENT == capi.FB_CONSISTENT
    assert (temporal.SUPPORT_PREV, temporal.SUPPORT_NEXT) == (1, 2)


def test_the_header_states_the_two_consequences():
    section = abi.section("Motion-compensated temporal filtering", "int ofdis_batch_temporal_filter")
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
    p = abi.ptr
    return capi.lib().ofdis_temporal_filter(p(hb.frames, frames), p(hb.flow, fw), p(hb.flow, rev), hb.mask.ctypes.data,
                                            hb.mask.ctypes.data, p(hb.frames, True) if in_place else p(hb.out, out),
                                            hb.support.ctypes.data, npairs, w, h, noc, wn, tau, None)


@pytest.mark.parametrize("which", ["frames", "fw", "rev", "out"])
def test_temporal_filter_rejects_null_pointers(which):
    abi.rejected(_filter(_Host(), **{which: False}))


def test_temporal_filter_rejects_in_place():
    abi.rejected(_filter(_Host(), in_place=True), "in place")


@pytest.mark.parametrize("noc", [0, 2, 4, -1])
def test_temporal_filter_rejects_noc(noc):
    abi.rejected(_filter(_Host(noc=3), noc=noc), "noc")


@pytest.mark.parametrize("npairs,w,h", [(0, 8, 4), (-1, 8, 4), (2, 0, 4), (2, 8, 0), (2, -8, 4), (2, 1 << 16, 1 << 16)])
def test_temporal_filter_rejects_bad_sizes(npairs, w, h):
    abi.rejected(_filter(_Host(), npairs=npairs, w=w, h=h), "size")


@pytest.mark.parametrize("wn", [-1e-7, 1.0000001, 2.0, -1.0, math.nan, math.inf, -math.inf])
def test_temporal_filter_rejects_wn(wn):
    abi.rejected(_filter(_Host(), wn=wn), "wn")


@pytest.mark.parametrize("tau", [0.0, -0.0, -1.0, -math.inf, math.nan, FLT_MIN / 2, 1e-45])
def test_temporal_filter_rejects_tau(tau):
    abi.rejected(_filter(_Host(), tau=tau), "tau")


def test_the_value_checks_accept_their_closed_ranges():
    """both ends of [0, 1] and -0.0 for wn; +inf, FLT_MIN and FLT_MAX for tau: the call gets as far as the size check"""
    for wn in (0.0, -0.0, 1.0, 0.5, 1e-30):
        abi.rejected(_filter(_Host(), wn=wn, npairs=0), "size")
    for tau in (math.inf, FLT_MIN, float(np.finfo(_f32).max), 1.5):
        abi.rejected(_filter(_Host(), tau=tau, npairs=0), "size")


def test_batch_temporal_filter_without_a_context():
    hb = _Host()
    rc = capi.lib().ofdis_batch_temporal_filter(None, hb.frames.ctypes.data, 0, 2, hb.out.ctypes.data, None, 8, 4, 1.0, math.inf,
                                                capi.FB_ALPHA, capi.FB_BETA, None)
    abi.rejected(rc)
