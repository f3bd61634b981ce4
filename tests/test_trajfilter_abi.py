"""CPU: the trajectory-filter entry points (include/ofdis.h: ofdis_trajectory_filter, ofdis_batch_trajectory_filter) in the header,
the binding and the export list, and their argument checks that return before any device work.  Host buffers stand in for the
device arrays: every call here returns before it would launch.  The kernels, and the checks that need a context (creating one
needs a device): tests/test_gpu_trajfilter.py."""
import math
import re

import numpy as np
import pytest

import abi
from of_dis_amd import capi
from seq_products import FLT_MIN

_f32 = np.float32


def test_the_header_states_the_consequences():
    section = abi.section("Temporal filtering along flow trajectories", "int ofdis_batch_trajectory_filter")
    for words in ("Radius 1 matches the existing filter", "Zero weights return the clip",
                  r"Identical frames with zero flows return\s+\*?\s*themselves", "Reach matches a track",
                  r"A photometric gate of 0 does not end a\s+\*?\s*direction"):
        assert re.search(words, section), words


class _Host:
    """host stand-ins for a 2-pair 8x4 case"""

    def __init__(self, w=8, h=4, npairs=2, noc=1):
        self.frames = np.zeros((npairs + 1, h, w, noc), np.uint8)
        self.flow = np.zeros((npairs, h, w, 2), _f32)
        self.out = np.zeros((npairs + 1, h, w, noc), np.uint8)
        self.support = np.zeros((npairs + 1, h, w), np.uint8)


def _filter(hb, frames=True, fw=True, rev=True, out=True, in_place=False, npairs=2, w=8, h=4, noc=1, weights=(1.0, 0.5),
            radius=None, tau=math.inf, fb_check=1, alpha=capi.FB_ALPHA, beta=capi.FB_BETA):
    p = abi.ptr
    wts = None if weights is None else np.asarray(weights, _f32)
    return capi.lib().ofdis_trajectory_filter(p(hb.frames, frames), p(hb.flow, fw), p(hb.flow, rev),
                                              p(hb.frames, True) if in_place else p(hb.out, out), hb.support.ctypes.data,
                                              npairs, w, h, noc, None if wts is None else wts.ctypes.data,
                                              len(weights) if radius is None else radius, tau, fb_check, alpha, beta, None)


@pytest.mark.parametrize("which", ["frames", "fw", "rev", "out"])
def test_rejects_null_pointers(which):
    abi.rejected(_filter(_Host(), **{which: False}))


def test_rejects_null_weights():
    abi.rejected(_filter(_Host(), weights=None, radius=2), "weights")


def test_rejects_in_place():
    abi.rejected(_filter(_Host(), in_place=True), "in place")


@pytest.mark.parametrize("noc", [0, 2, 4, -1])
def test_rejects_noc(noc):
    abi.rejected(_filter(_Host(noc=3), noc=noc), "noc")


@pytest.mark.parametrize("npairs,w,h", [(0, 8, 4), (-1, 8, 4), (2, 0, 4), (2, 8, 0), (2, -8, 4), (2, 1 << 16, 1 << 16)])
def test_rejects_bad_sizes(npairs, w, h):
    abi.rejected(_filter(_Host(), npairs=npairs, w=w, h=h), "size")


@pytest.mark.parametrize("radius", [0, -1, 9, 1 << 30])
def test_rejects_radius(radius):
    abi.rejected(_filter(_Host(), weights=[1.0] * 16, radius=radius), "radius")


@pytest.mark.parametrize("bad", [-1e-7, 1.0000001, 2.0, -1.0, math.nan, math.inf, -math.inf])
@pytest.mark.parametrize("at", [0, 1, 7])
def test_rejects_a_weight(bad, at):
    weights = [0.5] * 8
    weights[at] = bad
    abi.rejected(_filter(_Host(), weights=weights), "weight")


def test_weights_beyond_the_radius_are_not_read():
    """radius 2 of an array whose third entry is out of range: the call gets as far as the size check"""
    abi.rejected(_filter(_Host(), weights=[1.0, 0.0, 7.0], radius=2, npairs=0), "size")


@pytest.mark.parametrize("tau", [0.0, -0.0, -1.0, -math.inf, math.nan, FLT_MIN / 2, 1e-45])
def test_rejects_tau(tau):
    abi.rejected(_filter(_Host(), tau=tau), "tau")


@pytest.mark.parametrize("fb_check", [-1, 2, 255])
def test_rejects_fb_check(fb_check):
    abi.rejected(_filter(_Host(), fb_check=fb_check), "fb_check")


@pytest.mark.parametrize("kw", [dict(alpha=-0.01), dict(beta=-0.5), dict(alpha=math.nan), dict(beta=math.inf), dict(alpha=math.inf),
                                dict(beta=math.nan)], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
@pytest.mark.parametrize("fb_check", [0, 1])
def test_rejects_alpha_and_beta(kw, fb_check):
    abi.rejected(_filter(_Host(), fb_check=fb_check, **kw), "alpha")


def test_the_value_checks_accept_their_closed_ranges():
    """both ends of [0, 1] and -0.0 for a weight, radius 1 and 8, +inf, FLT_MIN and FLT_MAX for tau, fb_check 0 and 1, alpha =
    beta = 0: the call gets as far as the size check"""
    for weights in ([0.0], [-0.0, 1.0], [1e-30] * 8, [1.0] * 8):
        abi.rejected(_filter(_Host(), weights=weights, npairs=0), "size")
    for tau in (math.inf, FLT_MIN, float(np.finfo(_f32).max), 1.5):
        abi.rejected(_filter(_Host(), tau=tau, npairs=0), "size")
    for fb_check in (0, 1):
        abi.rejected(_filter(_Host(), fb_check=fb_check, alpha=0.0, beta=0.0, npairs=0), "size")


def test_batch_form_without_a_context():
    hb = _Host()
    wts = np.ones(2, _f32)
    rc = capi.lib().ofdis_batch_trajectory_filter(None, hb.frames.ctypes.data, 0, 2, hb.out.ctypes.data, None, 8, 4,
                                                  wts.ctypes.data, 2, math.inf, 1, capi.FB_ALPHA, capi.FB_BETA, None)
    abi.rejected(rc)
