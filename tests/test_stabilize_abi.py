"""CPU: the stabilisation entry points (include/ofdis.h: ofdis_camera_path, ofdis_warp_frames, ofdis_batch_stabilize) in the
header, the binding and the export list, and the argument checks of the two stand-alone calls, which return before any device
work.  Host buffers stand in for the device arrays: every call here returns before it would launch.  The kernels, and the
checks that need a context (creating one needs a device): tests/test_gpu_stabilize.py."""
import math
import re

import numpy as np
import pytest

import abi
from of_dis_amd import capi

_p = abi.ptr


def test_the_header_states_the_definition_and_its_consequences():
    section = re.sub(r"\s+\*?\s*", " ", abi.section("Video stabilisation: ", "#define OFDIS_STAB_MAX_RADIUS"))
    for phrase in ("a zero warp returns the frame bit for bit", "integer translation", "zeros on the uncovered border",
                   "truncated symmetrically", "a uniform pan is left alone", "relative to frame f", "HOST array",
                   "homography", "rolling-shutter", "inpainting", "sequence driver", "stereo contexts",
                   "of_dis_amd/stabilize.py"):
        assert phrase in section, phrase
    # the global-motion section points here
    gm = abi.section("Global (camera) motion models", "#define OFDIS_GM_MAX_SIDE")
    assert '"Video stabilisation"' in gm and "stabilisation itself" in gm


# ------------------------------------------------------------------ argument checks
class _Host:
    """host stand-ins for a 3-pair / 4-frame 8x4 case"""

    def __init__(self, w=8, h=4, n=4, noc=1):
        self.models = np.zeros((n - 1, 6), np.float64)
        self.warps = np.zeros((n, 6), np.float64)
        self.weights = np.ones(capi.STAB_MAX_RADIUS + 2, np.float64)
        self.frames = np.zeros((n, h, w, noc), np.uint8)
        self.out = np.zeros((n, h, w, noc), np.uint8)
        self.inside = np.zeros((n, h, w), np.uint8)


def _path(hb, models=True, weights=True, warps=True, npairs=3, radius=2, zoom=1.0):
    return capi.lib().ofdis_camera_path(_p(hb.models, models), npairs, _p(hb.weights, weights), radius, zoom, _p(hb.warps, warps),
                                        None)


def _warp(hb, frames=True, warps=True, out=True, inside=True, in_place=False, n=4, w=8, h=4, noc=1, border=0):
    optr = _p(hb.frames) if in_place else _p(hb.out, out)
    return capi.lib().ofdis_warp_frames(_p(hb.frames, frames), _p(hb.warps, warps), optr, _p(hb.inside, inside), n, w, h, noc,
                                        border, None)


@pytest.mark.parametrize("which", ["models", "weights", "warps"])
def test_camera_path_null_pointers(which):
    abi.rejected(_path(_Host(), **{which: False}))


@pytest.mark.parametrize("radius", [-1, 65, 1 << 20])
def test_camera_path_rejects_radius(radius):
    abi.rejected(_path(_Host(), radius=radius), "radius")


@pytest.mark.parametrize("j,value", [(0, 0.0), (0, -1.0), (0, math.nan), (0, math.inf), (1, -1e-300), (2, math.nan), (2, math.inf),
                                     (2, -math.inf)])
def test_camera_path_rejects_weights(j, value):
    hb = _Host()
    hb.weights[j] = value
    abi.rejected(_path(hb), "weights")


def test_camera_path_reads_radius_plus_one_weights():
    """a bad value past the window is not looked at: the call gets as far as the size check"""
    hb = _Host()
    hb.weights[3] = math.nan
    abi.rejected(_path(hb, radius=2, npairs=0), "npairs")
    abi.rejected(_path(hb, radius=3, npairs=0), "weights")
    hb = _Host()
    hb.weights[1:] = 0.0                                   # zeros are allowed past w_0
    abi.rejected(_path(hb, radius=64, npairs=0), "npairs")


@pytest.mark.parametrize("zoom", [0.0, 0.999, -1.0, 16.001, math.nan, math.inf, -math.inf])
def test_camera_path_rejects_zoom(zoom):
    abi.rejected(_path(_Host(), zoom=zoom), "zoom")


@pytest.mark.parametrize("npairs", [0, -1, -(1 << 30)])
def test_camera_path_rejects_npairs(npairs):
    abi.rejected(_path(_Host(), npairs=npairs), "npairs")


def test_camera_path_value_checks_accept_their_ranges():
    for kw in (dict(radius=0), dict(radius=64), dict(zoom=1.0), dict(zoom=16.0)):
        abi.rejected(_path(_Host(), npairs=0, **kw), "npairs")


@pytest.mark.parametrize("which", ["frames", "warps", "out"])
def test_warp_frames_null_pointers(which):
    abi.rejected(_warp(_Host(), **{which: False}))


def test_warp_frames_rejects_in_place():
    abi.rejected(_warp(_Host(), in_place=True), "in place")


@pytest.mark.parametrize("noc", [0, 2, 4, -1])
def test_warp_frames_rejects_noc(noc):
    abi.rejected(_warp(_Host(), noc=noc), "noc")


@pytest.mark.parametrize("border", [-1, 2, 3, 1 << 20])
def test_warp_frames_rejects_border(border):
    abi.rejected(_warp(_Host(), border=border), "border")


SIZES = [(0, 8, 4), (-1, 8, 4), (2, 0, 4), (2, 8, 0), (2, -8, 4), (2, 1 << 16, 1 << 16), (2, 8193, 4), (2, 8, 8193)]


@pytest.mark.parametrize("n,w,h", SIZES)
def test_warp_frames_rejects_bad_sizes(n, w, h):
    abi.rejected(_warp(_Host(), n=n, w=w, h=h), "size")


def test_warp_frames_value_checks_accept_their_ranges():
    """both borders, both channel counts, inside = NULL: the call gets as far as the size check"""
    for kw in (dict(border=0), dict(border=1), dict(noc=1), dict(noc=3), dict(inside=False)):
        abi.rejected(_warp(_Host(), n=0, **kw), "size")


def test_batch_stabilize_without_a_context():
    hb = _Host()
    abi.rejected(capi.lib().ofdis_batch_stabilize(None, _p(hb.frames), 0, 3, 1, 3, 1.0, 0, capi.FB_ALPHA, capi.FB_BETA, _p(hb.weights),
                                               2, 1.0, 0, _p(hb.out), _p(hb.inside), _p(hb.warps), 8, 4, None))
