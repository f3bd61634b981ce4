"""CPU: the projective stabilisation entry points (include/ofdis.h: ofdis_camera_path_projective, ofdis_warp_frames_projective,
ofdis_batch_stabilize_projective) in the header and the binding, and the argument checks of the two stand-alone calls, which
return before any device work.  Host buffers stand in for the device arrays: every call here returns before it would launch.
The kernels, and the checks that need a context: tests/test_gpu_stabilize_projective.py."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import abi
from of_dis_amd import capi, stabilize
from of_dis_amd.abi import prototypes

_p = abi.ptr
_I, _F, _D, _P = C.c_int, C.c_float, C.c_double, C.c_void_p


def test_the_three_calls_are_declared_as_the_issue_states_them():
    proto = prototypes()
    assert proto["ofdis_camera_path_projective"] == (_I, [_P, _I, _I, _I, _P, _I, _D, _P, _P])
    assert proto["ofdis_warp_frames_projective"] == (_I, [_P] * 4 + [_I] * 5 + [_P])
    assert proto["ofdis_batch_stabilize_projective"] == (_I, [_P, _P, _I, _I, _I, _F, _I, _F, _F, _P, _I, _D, _I, _P, _P, _P, _I, _I, _P])
    # ... which is ofdis_batch_stabilize's without `model`
    affine = proto["ofdis_batch_stabilize"][1]
    assert proto["ofdis_batch_stabilize_projective"][1] == affine[:4] + affine[5:]
    for name in ("ofdis_camera_path_projective", "ofdis_warp_frames_projective", "ofdis_batch_stabilize_projective"):
        assert name in abi.exported() and getattr(capi.lib(), name).argtypes is not None


def test_the_header_states_the_definition_and_its_consequences():
    section = re.sub(r"\s+\*?\s*", " ", abi.section("Projective video stabilisation: ", "int ofdis_camera_path_projective"))
    for phrase in ("[[1+g1, g2, g0], [g4, 1+g5, g3], [-g6, -g7, 1]]", "T_k = (1 + a1, a2, a4, 1 + a5, a0, a3, 0 - a6, 0 - a7)",
                   "(1 - |M.gx|*hx) - |M.gy|*hy >= 0.5", "a = (T.a*M.a + T.b*M.c) + T.tx*M.gx", "n = (T.gx*M.tx + T.gy*M.ty) + 1",
                   "tx = (T.b*T.ty - T.tx*T.d) / D", "gy = (T.b*T.gx - T.a*T.gy) / D", "word for word those of ofdis_camera_path",
                   "usable(Q) and usable(inv(Q))", "g6 = 0 - W.gx*s", "DISPLACEMENT form", "r = 1.0f / D",
                   "one correctly rounded division per pixel", "mu = ((gf0 + gf1*xc) + gf2*yc) + e*xc", "ins = D > 0 and inside(p)",
                   "equals ofdis_warp_frames on g0 .. g5", "A zero warp returns the frame bit for bit", "integer translation",
                   "g6 = g7 = 0 exactly", "to rounding, not to the bit", "a DLT fit", "similarity models", "rolling-shutter",
                   "automatic crop", "C++ sequence driver", "camera_path_projective_ref", "warp_frames_projective_ref"):
        assert phrase in section, phrase
    # the sections that said homography stabilisation is not provided point here instead
    flat = re.sub(r"\s+\*?\s*", " ", abi.header())
    assert flat.count('"Projective video stabilisation"') >= 2
    for l in re.findall(r"Not provided[^.]*\.", flat):
        assert "homography and similarity" not in l and "stay affine" not in l, l
    assert stabilize.STAB_MIN_DENOM == capi.STAB_MIN_DENOM == 0.5


# ------------------------------------------------------------------ argument checks
class _Host:
    """host stand-ins for a 3-pair / 4-frame 8x4 case"""

    def __init__(self, w=8, h=4, n=4, noc=1):
        self.models = np.zeros((n - 1, 8), np.float64)
        self.warps = np.zeros((n, 8), np.float64)
        self.weights = np.ones(capi.STAB_MAX_RADIUS + 2, np.float64)
        self.frames = np.zeros((n, h, w, noc), np.uint8)
        self.out = np.zeros((n, h, w, noc), np.uint8)
        self.inside = np.zeros((n, h, w), np.uint8)


def _path(hb, models=True, weights=True, warps=True, npairs=3, w=8, h=4, radius=2, zoom=1.0):
    return capi.lib().ofdis_camera_path_projective(_p(hb.models, models), npairs, w, h, _p(hb.weights, weights), radius, zoom,
                                                   _p(hb.warps, warps), None)


def _warp(hb, frames=True, warps=True, out=True, inside=True, in_place=False, n=4, w=8, h=4, noc=1, border=0):
    optr = _p(hb.frames) if in_place else _p(hb.out, out)
    return capi.lib().ofdis_warp_frames_projective(_p(hb.frames, frames), _p(hb.warps, warps), optr, _p(hb.inside, inside), n, w,
                                                   h, noc, border, None)


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
    hb = _Host()
    hb.weights[3] = math.nan
    abi.rejected(_path(hb, radius=2, npairs=0), "npairs")
    abi.rejected(_path(hb, radius=3, npairs=0), "weights")


@pytest.mark.parametrize("zoom", [0.0, 0.999, -1.0, 16.001, math.nan, math.inf, -math.inf])
def test_camera_path_rejects_zoom(zoom):
    abi.rejected(_path(_Host(), zoom=zoom), "zoom")


@pytest.mark.parametrize("npairs", [0, -1, -(1 << 30)])
def test_camera_path_rejects_npairs(npairs):
    abi.rejected(_path(_Host(), npairs=npairs), "npairs")


@pytest.mark.parametrize("w,h", [(0, 4), (8, 0), (-8, 4), (8, -1), (8193, 4), (8, 8193), (1 << 30, 1 << 30)])
def test_camera_path_rejects_sides(w, h):
    abi.rejected(_path(_Host(), w=w, h=h), "size")


def test_camera_path_value_checks_accept_their_ranges():
    for kw in (dict(radius=0), dict(radius=64), dict(zoom=1.0), dict(zoom=16.0), dict(w=1, h=1), dict(w=8192, h=8192)):
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


@pytest.mark.parametrize("n,w,h", [(0, 8, 4), (-1, 8, 4), (2, 0, 4), (2, 8, 0), (2, -8, 4), (2, 1 << 16, 1 << 16), (2, 8193, 4),
                                   (2, 8, 8193)])
def test_warp_frames_rejects_bad_sizes(n, w, h):
    abi.rejected(_warp(_Host(), n=n, w=w, h=h), "size")


def test_warp_frames_value_checks_accept_their_ranges():
    for kw in (dict(border=0), dict(border=1), dict(noc=1), dict(noc=3), dict(inside=False)):
        abi.rejected(_warp(_Host(), n=0, **kw), "size")


def test_batch_stabilize_projective_without_a_context():
    hb = _Host()
    abi.rejected(capi.lib().ofdis_batch_stabilize_projective(None, _p(hb.frames), 0, 3, 3, 1.0, 0, capi.FB_ALPHA, capi.FB_BETA,
                                                             _p(hb.weights), 2, 1.0, 0, _p(hb.out), _p(hb.inside), _p(hb.warps),
                                                             8, 4, None))
