"""CPU: the projective entry points (include/ofdis.h: ofdis_projective_motion_work_bytes, ofdis_projective_motion,
ofdis_projective_compensate, the two ofdis_batch_* twins and ofdis_track_select_projective) in the header and the binding, and
their argument checks, which return before any device work -- every rejection the 6-parameter twins make
(tests/test_gmotion_abi.py, tests/test_track_select_abi.py).  Host buffers stand in for the device arrays: every call here
returns before it would launch.  The kernels: tests/test_gpu_projective.py."""
import ctypes as C
import functools
import math
import re

import numpy as np
import pytest

import abi
from camera_cases import BAD_SIZES, Host, host_compensate, host_fit
from of_dis_amd import capi
from of_dis_amd.abi import prototypes

_f32 = np.float32
_p = abi.ptr
RECORD = 24 * 8


def test_the_header_states_the_model_and_what_is_out_of_scope():
    section = re.sub(r"\s+\*?\s*", " ", abi.section("Projective camera models: the 8-parameter", "size_t ofdis_projective_motion_work_bytes"))
    for text in ("not a DLT homography fit", "overflow 64 bits for a single pixel", "[[1+a1, a2, a0], [a4, 1+a5, a3], [-a6, -a7, 1]]",
                 "ofdis_batch_stabilize stay affine", "not closed under composition", "similarity models", "RANSAC",
                 "C++ sequence driver", "2^-40", "128 bits", "CORRECTLY ROUNDED", "L D L^T", "8, 6 (affine), 2 (translation) or 0"):
        assert text in section, text
    # the Not-provided lists: homography models have left those of global motion and track selection, not stabilisation's
    flat = re.sub(r"\s+\*?\s*", " ", abi.header())
    lists = re.findall(r"Not provided[^.]*\.", flat)
    with_h = [l for l in lists if "homography" in l]
    assert len(with_h) == 1 and "rolling-shutter" in with_h[0], with_h
    assert sum("similarity" in l for l in lists) >= 3


def test_signatures():
    P = prototypes()
    i, f, p, z = C.c_int, C.c_float, C.c_void_p, C.c_size_t
    assert P["ofdis_projective_motion_work_bytes"] == (z, [i, i, i])
    assert P["ofdis_projective_motion"] == (i, [p, p, i, i, i, i, f, p, p, p, z, p])
    assert P["ofdis_projective_compensate"] == (i, [p, p, p, i, i, i, f, p, p, p])
    assert P["ofdis_batch_projective_motion"] == (i, [p, i, i, i, f, i, f, f, p, p, i, i, p])
    assert P["ofdis_batch_projective_compensate"] == (i, [p, i, i, p, f, i, f, f, p, p, i, i, p])
    assert P["ofdis_track_select_projective"] == P["ofdis_track_select"]   # the argument list of ofdis_track_select
    # the 6-parameter fit goes on rejecting model = 2: the feature adds no model code
    assert abi.enumerator("OFDIS_GM_AFFINE") == 1 and "OFDIS_GM_PROJECTIVE" not in abi.enumerators()


# ------------------------------------------------------------------ ofdis_projective_motion_work_bytes
def test_work_bytes():
    wb = capi.lib().ofdis_projective_motion_work_bytes
    assert wb(1, 1, 1) == RECORD                                 # one workgroup, one record of 24 x 8 bytes
    assert wb(1, 256, 112) == RECORD * ((64 * 112 + 255) // 256)
    sizes = [wb(n, 300, 70) for n in (1, 2, 3, 10, 1000)]
    assert all(s > 0 for s in sizes) and sizes == sorted(set(sizes)) and sizes[3] == 10 * sizes[0]
    assert wb(1, 8192, 8192) == RECORD * (2048 * 8192 // 256)
    for n, w, h in ((1, 1, 1), (3, 300, 70), (2, 8192, 2)):      # the records of the affine fit, twice as wide
        assert wb(n, w, h) == 2 * capi.lib().ofdis_global_motion_work_bytes(n, w, h)
    for bad in ((0, 8, 4), (-1, 8, 4), (1, 0, 4), (1, 8, 0), (1, -8, 4), (1, 8193, 4), (1, 4, 8193), (1, 1 << 16, 1 << 16)):
        assert wb(*bad) == 0, bad


# ------------------------------------------------------------------ argument checks
# the host stand-ins and the two calls: tests/camera_cases.py, shared with the other model order
_Host = functools.partial(Host, 8)
_fit, _comp = host_fit, host_compensate


@pytest.mark.parametrize("which", ["flow", "models"])
def test_null_pointers(which):
    abi.rejected(_fit(_Host(), **{which: False}))
    abi.rejected(_comp(_Host(), **{which: False}))


def test_compensate_needs_an_output():
    abi.rejected(_comp(_Host(), residual=False, label=False))


@pytest.mark.parametrize("rounds", [0, -1, 9, 1 << 20])
def test_rejects_rounds(rounds):
    abi.rejected(_fit(_Host(), rounds=rounds), "rounds")


@pytest.mark.parametrize("thresh", [0.0, -0.0, -1.0, math.nan, math.inf, -math.inf])
def test_rejects_thresh(thresh):
    abi.rejected(_fit(_Host(), thresh=thresh), "thresh")
    abi.rejected(_comp(_Host(), thresh=thresh), "thresh")


@pytest.mark.parametrize("npairs,w,h", BAD_SIZES)
def test_rejects_bad_sizes(npairs, w, h):
    abi.rejected(_fit(_Host(), npairs=npairs, w=w, h=h), "size")
    abi.rejected(_comp(_Host(), npairs=npairs, w=w, h=h), "size")


def test_rejects_the_work_buffer():
    need = capi.lib().ofdis_projective_motion_work_bytes(2, 8, 4)
    assert need == 2 * RECORD
    abi.rejected(_fit(_Host(), work=False), "work")
    abi.rejected(_fit(_Host(), work_bytes=need - 1), "work")
    abi.rejected(_fit(_Host(), work_bytes=capi.lib().ofdis_global_motion_work_bytes(2, 8, 4)), "ofdis_projective_motion_work_bytes")
    abi.rejected(_fit(_Host(), work_bytes=0), "work")
    abi.rejected(_fit(_Host(), work_off=4), "work")


def test_the_value_checks_accept_their_ranges():
    """rounds 1 and 8, tiny and huge thresholds, the largest side: the call gets as far as the work-buffer check"""
    for kw in (dict(rounds=1), dict(rounds=8), dict(thresh=1e-30), dict(thresh=3e38), dict(w=8192, h=1), dict(w=1, h=8192)):
        abi.rejected(_fit(_Host(), work=False, **kw), "work")


def test_batch_calls_without_a_context():
    hb = _Host()
    L = capi.lib()
    abi.rejected(L.ofdis_batch_projective_motion(None, 0, 2, 3, 1.0, 0, capi.FB_ALPHA, capi.FB_BETA, _p(hb.models), _p(hb.stats), 8,
                                                 4, None))
    abi.rejected(L.ofdis_batch_projective_compensate(None, 0, 2, _p(hb.models), 1.0, 0, capi.FB_ALPHA, capi.FB_BETA,
                                                     _p(hb.residual), _p(hb.label), 8, 4, None))


def test_global_motion_still_rejects_model_2():
    hb = _Host()
    six = np.zeros((2, 6), np.float64)
    rc = capi.lib().ofdis_global_motion(_p(hb.flow), _p(hb.mask), 2, 8, 4, 2, 3, 1.0, _p(six), _p(hb.stats), _p(hb.work),
                                        hb.work.nbytes, None)
    abi.rejected(rc, "model")


# ------------------------------------------------------------------ ofdis_track_select_projective
class _Tracks:
    def __init__(self, n=4, lmax=3):
        self.tracks = np.zeros((lmax + 1, n, 2), _f32)
        self.start, self.len = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.info = np.array([n, 0], np.int64)
        self.models = np.zeros((lmax, 8), np.float64)
        self.tracks_out, self.start_out, self.len_out = self.tracks.copy(), self.start.copy(), self.len.copy()
        self.info_out = np.zeros(2, np.int64)
        self.work = np.zeros(64, np.int64)
        self.n, self.lmax = n, lmax


def _select(t, off=(), lmax=None, max_tracks=None, max_out=None, npairs=3, w=640, h=480, params=None, work=True, work_bytes=None,
            work_off=0, no_params=False):
    p = capi.TrackSelectParams.of(params)
    on = lambda name: _p(getattr(t, name), name not in off)
    wb = t.work.nbytes - 8 if work_bytes is None else work_bytes
    return capi.lib().ofdis_track_select_projective(
        on("tracks"), on("start"), on("len"), on("info"), t.lmax if lmax is None else lmax, t.n if max_tracks is None else max_tracks,
        on("models"), npairs, w, h, None if no_params else C.byref(p), None, None, t.n if max_out is None else max_out,
        on("tracks_out"), on("start_out"), on("len_out"), on("info_out"), None, None,
        t.work.ctypes.data + work_off if work else None, wb, None)


@pytest.mark.parametrize("name", ["tracks", "start", "len", "info", "tracks_out", "start_out", "len_out", "info_out"])
def test_track_select_null_pointers(name):
    abi.rejected(_select(_Tracks(), off=(name,)), name)


def test_track_select_rejections():
    t = _Tracks()
    abi.rejected(_select(t, no_params=True), "params")
    abi.rejected(_select(t, lmax=0), "lmax")
    for bad in (0, -1, (1 << 24) + 1):
        abi.rejected(_select(t, max_tracks=bad), "max_tracks")
        abi.rejected(_select(t, max_out=bad), "max_tracks_out")
    for kw in (dict(npairs=0), dict(w=0), dict(h=0), dict(w=8193), dict(h=8193)):
        abi.rejected(_select(t, **kw), "models")
    mk = capi.TrackSelectParams
    for params, word in ((mk(min_len=-1), "min_len"), (mk(min_std=-1.0), "min_std"), (mk(min_std=math.inf), "min_std"),
                         (mk(max_std=math.nan), "max_std"), (mk(max_step=-1.0), "max_step"), (mk(max_step_share=1.5), "max_step_share"),
                         (mk(min_camera=math.nan), "min_camera"), (mk(min_camera=math.inf), "min_camera"), (mk(tests=0x40), "tests")):
        abi.rejected(_select(t, params=params), word)
    abi.rejected(_select(t, work=False), "work")
    abi.rejected(_select(t, work_bytes=capi.track_select_work_bytes(t.n) - 1), "work")
    abi.rejected(_select(t, work_off=4), "work")
    # without models the sizes are not looked at: the call gets as far as the work buffer
    abi.rejected(_select(t, off=("models",), npairs=0, w=0, h=0, work=False), "work")
