"""CPU: the stabilisation entry points (include/ofdis.h: ofdis_camera_path, ofdis_warp_frames, ofdis_batch_stabilize) in the
header, the binding and the export list, and the argument checks of the two stand-alone calls, which return before any device
work.  Host buffers stand in for the device arrays: every call here returns before it would launch.  The kernels, and the
checks that need a context (creating one needs a device): tests/test_gpu_stabilize.py."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from of_dis_amd import build, capi, stabilize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
SYMBOLS = ["ofdis_camera_path", "ofdis_warp_frames", "ofdis_batch_stabilize"]


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
    ctype = {"float": capi.C.c_float, "int": capi.C.c_int, "double": capi.C.c_double}

    def want(arg):
        words = arg.replace("*", " * ").split()
        if "*" in words:   # const uint8_t*, uint8_t*, const double*, double*, void*, ofdis_batch*
            assert words[-2] == "*" and words[0] in ("const", "uint8_t", "double", "void", "ofdis_batch"), arg
            return capi.VP
        assert len(words) == 2, arg
        return ctype[words[0]]

    for name in SYMBOLS:
        args = re.search(r"\bint " + name + r"\s*\((.*?)\)\s*;", src, re.S).group(1)
        assert getattr(capi.lib(), name).argtypes == [want(a) for a in args.split(",")], name
    flat = re.sub(r"\s+", " ", src)
    assert "const double* weights , int radius, double zoom" in flat   # (the weights are a host array, said in a comment)
    assert "uint8_t* out, uint8_t* inside , double* warps , int width_org, int height_org, void* stream" in flat


def test_the_version_stays():
    assert int(re.search(r"#define OFDIS_VERSION (\d+)", _header()).group(1)) == capi.OFDIS_VERSION == 3


def test_constants_match_the_binding():
    hdr = _header()
    define = lambda name: re.search(r"#define " + name + r"\s+([0-9.]+)f?\s", hdr).group(1)
    assert int(define("OFDIS_STAB_MAX_RADIUS")) == capi.STAB_MAX_RADIUS == stabilize.STAB_MAX_RADIUS == 64
    assert float(define("OFDIS_STAB_MIN_DET")) == capi.STAB_MIN_DET == stabilize.STAB_MIN_DET == 0.25
    assert float(define("OFDIS_STAB_MAX_DET")) == capi.STAB_MAX_DET == stabilize.STAB_MAX_DET == 4.0
    assert float(define("OFDIS_STAB_MAX_ZOOM")) == capi.STAB_MAX_ZOOM == stabilize.STAB_MAX_ZOOM == 16.0
    enum = lambda name: int(re.search(r"\b" + name + r" = (\d+)", hdr).group(1))
    assert enum("OFDIS_BORDER_CONSTANT") == capi.BORDER_CONSTANT == stabilize.BORDER_CONSTANT == 0
    assert enum("OFDIS_BORDER_REPLICATE") == capi.BORDER_REPLICATE == stabilize.BORDER_REPLICATE == 1
    assert stabilize.GM_MAX_SIDE == capi.GM_MAX_SIDE


def test_the_header_states_the_definition_and_its_consequences():
    hdr = _header()
    section = re.sub(r"\s+\*?\s*", " ", hdr[hdr.index("Video stabilisation: "):hdr.index("#define OFDIS_STAB_MAX_RADIUS")])
    for phrase in ("a zero warp returns the frame bit for bit", "integer translation", "zeros on the uncovered border",
                   "truncated symmetrically", "a uniform pan is left alone", "relative to frame f", "HOST array",
                   "homography", "rolling-shutter", "inpainting", "sequence driver", "stereo contexts",
                   "of_dis_amd/stabilize.py"):
        assert phrase in section, phrase
    # the global-motion section points here
    gm = hdr[hdr.index("Global (camera) motion models"):hdr.index("#define OFDIS_GM_MAX_SIDE")]
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


def _p(a, on=True):
    return a.ctypes.data if on else None


def _path(hb, models=True, weights=True, warps=True, npairs=3, radius=2, zoom=1.0):
    return capi.lib().ofdis_camera_path(_p(hb.models, models), npairs, _p(hb.weights, weights), radius, zoom, _p(hb.warps, warps),
                                        None)


def _warp(hb, frames=True, warps=True, out=True, inside=True, in_place=False, n=4, w=8, h=4, noc=1, border=0):
    optr = _p(hb.frames) if in_place else _p(hb.out, out)
    return capi.lib().ofdis_warp_frames(_p(hb.frames, frames), _p(hb.warps, warps), optr, _p(hb.inside, inside), n, w, h, noc,
                                        border, None)


def _rejected(rc, word=None):
    assert rc == INVALID
    msg = capi.lib().ofdis_last_error().decode()
    assert msg and (word is None or word in msg), msg


@pytest.mark.parametrize("which", ["models", "weights", "warps"])
def test_camera_path_null_pointers(which):
    _rejected(_path(_Host(), **{which: False}))


@pytest.mark.parametrize("radius", [-1, 65, 1 << 20])
def test_camera_path_rejects_radius(radius):
    _rejected(_path(_Host(), radius=radius), "radius")


@pytest.mark.parametrize("j,value", [(0, 0.0), (0, -1.0), (0, math.nan), (0, math.inf), (1, -1e-300), (2, math.nan), (2, math.inf),
                                     (2, -math.inf)])
def test_camera_path_rejects_weights(j, value):
    hb = _Host()
    hb.weights[j] = value
    _rejected(_path(hb), "weights")


def test_camera_path_reads_radius_plus_one_weights():
    """a bad value past the window is not looked at: the call gets as far as the size check"""
    hb = _Host()
    hb.weights[3] = math.nan
    _rejected(_path(hb, radius=2, npairs=0), "npairs")
    _rejected(_path(hb, radius=3, npairs=0), "weights")
    hb = _Host()
    hb.weights[1:] = 0.0                                   # zeros are allowed past w_0
    _rejected(_path(hb, radius=64, npairs=0), "npairs")


@pytest.mark.parametrize("zoom", [0.0, 0.999, -1.0, 16.001, math.nan, math.inf, -math.inf])
def test_camera_path_rejects_zoom(zoom):
    _rejected(_path(_Host(), zoom=zoom), "zoom")


@pytest.mark.parametrize("npairs", [0, -1, -(1 << 30)])
def test_camera_path_rejects_npairs(npairs):
    _rejected(_path(_Host(), npairs=npairs), "npairs")


def test_camera_path_value_checks_accept_their_ranges():
    for kw in (dict(radius=0), dict(radius=64), dict(zoom=1.0), dict(zoom=16.0)):
        _rejected(_path(_Host(), npairs=0, **kw), "npairs")


@pytest.mark.parametrize("which", ["frames", "warps", "out"])
def test_warp_frames_null_pointers(which):
    _rejected(_warp(_Host(), **{which: False}))


def test_warp_frames_rejects_in_place():
    _rejected(_warp(_Host(), in_place=True), "in place")


@pytest.mark.parametrize("noc", [0, 2, 4, -1])
def test_warp_frames_rejects_noc(noc):
    _rejected(_warp(_Host(), noc=noc), "noc")


@pytest.mark.parametrize("border", [-1, 2, 3, 1 << 20])
def test_warp_frames_rejects_border(border):
    _rejected(_warp(_Host(), border=border), "border")


SIZES = [(0, 8, 4), (-1, 8, 4), (2, 0, 4), (2, 8, 0), (2, -8, 4), (2, 1 << 16, 1 << 16), (2, 8193, 4), (2, 8, 8193)]


@pytest.mark.parametrize("n,w,h", SIZES)
def test_warp_frames_rejects_bad_sizes(n, w, h):
    _rejected(_warp(_Host(), n=n, w=w, h=h), "size")


def test_warp_frames_value_checks_accept_their_ranges():
    """both borders, both channel counts, inside = NULL: the call gets as far as the size check"""
    for kw in (dict(border=0), dict(border=1), dict(noc=1), dict(noc=3), dict(inside=False)):
        _rejected(_warp(_Host(), n=0, **kw), "size")


def test_batch_stabilize_without_a_context():
    hb = _Host()
    _rejected(capi.lib().ofdis_batch_stabilize(None, _p(hb.frames), 0, 3, 1, 3, 1.0, 0, capi.FB_ALPHA, capi.FB_BETA, _p(hb.weights),
                                               2, 1.0, 0, _p(hb.out), _p(hb.inside), _p(hb.warps), 8, 4, None))
