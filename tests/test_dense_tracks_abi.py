"""CPU: the dense-trajectory entry points (include/ofdis.h: ofdis_dense_tracks_cells, ofdis_dense_tracks_work_bytes,
ofdis_seed_texture, ofdis_dense_tracks, ofdis_batch_dense_tracks) in the header, the binding and the export list, and their
argument checks that return before any device work.  Host buffers stand in for the device arrays: every call here returns
before it would launch.  The kernels, and the checks that need a context (creating one needs a device):
tests/test_gpu_dense_tracks.py."""
import math
import re

import numpy as np
import pytest

import abi
from of_dis_amd import capi, tracking

_f32 = np.float32
_p = abi.ptr


def test_the_header_states_the_consequences():
    section = abi.section("Dense trajectories: the walk of ofdis_track_points", "int ofdis_batch_dense_tracks")
    for words in ("Replay:", "Coverage:", "Slot order:", "Known count:", r"4 \* \(2wr\+1\)\^2 \* noc", "is not provided",
                  "relies on no memset"):
        assert re.search(words, section), words


# ------------------------------------------------------------------ the grid and the work buffer
def test_cells_agree_with_the_numpy_grid():
    for w in range(2, 41):
        for h in range(2, 41):
            for stride in range(2, 10):
                got = capi.dense_tracks_cells(w, h, stride)
                want = tracking.dense_grid(w, h, stride) if min(w, h) >= stride else (0, 0)
                assert got == want, (w, h, stride, got, want)


def test_cells_take_null_pointers():
    assert capi.lib().ofdis_dense_tracks_cells(37, 11, 3, None, None) == 12 * 4


@pytest.mark.parametrize("w,h,stride", [(0, 8, 2), (8, 0, 2), (-8, 8, 2), (8, 8, 1), (8, 8, 0), (8, 8, 65), (8, 8, 9), (64, 63, 64),
                                        (1 << 16, 1 << 16, 2)])
def test_rejected_grids_have_no_cells_and_no_work_bytes(w, h, stride):
    assert capi.dense_tracks_cells(w, h, stride) == (0, 0)
    assert capi.lib().ofdis_dense_tracks_work_bytes(4, w, h, stride) == 0


@pytest.mark.parametrize("npairs", [0, -1])
def test_work_bytes_rejects_npairs(npairs):
    assert capi.lib().ofdis_dense_tracks_work_bytes(npairs, 64, 48, 2) == 0


def test_work_bytes_hold_the_stated_arrays():
    """the texture bits of every frame and cell, and 12 bytes of state for min(npairs * cells, OFDIS_DT_MAX_TRACKS) slots"""
    wb = capi.lib().ofdis_dense_tracks_work_bytes
    for npairs, w, h, stride in ((6, 64, 48, 2), (5, 37, 11, 3), (1024, 1024, 436, 5), (3, 9, 7, 4)):
        ncx, ncy = tracking.dense_grid(w, h, stride)
        slots = min(npairs * ncx * ncy, 1 << 24)
        got = wb(npairs, w, h, stride)
        assert got % 8 == 0 and got >= npairs * ncx * ncy + 12 * slots + 4 * (npairs + 1) + 4 * ncx * ncy
        assert got <= npairs * ncx * ncy + 12 * slots + 4 * (npairs + 1) + 5 * ncx * ncy + 128


# ------------------------------------------------------------------ argument checks
class _Host:
    """host stand-ins for a 2-pair 16x8 case"""

    def __init__(self, w=16, h=8, npairs=2, noc=1):
        self.frames = np.zeros((npairs + 1, h, w, noc), np.uint8)
        self.flow = np.zeros((npairs, h, w, 2), _f32)
        self.tracks = np.zeros((npairs + 1, 64, 2), _f32)
        self.start, self.len, self.info = np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(2, np.int64)
        self.work = np.zeros(1 << 16, np.uint8)  # (numpy allocates on 16-byte boundaries)
        self.out = np.zeros((npairs + 1, h, w), np.uint8)


def _dense(hb, frames=True, fw=True, rev=True, npairs=2, w=16, h=8, noc=1, stride=4, window=1, min_eig=5, max_len=0,
           alpha=capi.FB_ALPHA, beta=capi.FB_BETA, max_tracks=64, tracks=True, start=True, length=True, info=True, work=True,
           work_offset=0, work_bytes=None):
    wb = capi.lib().ofdis_dense_tracks_work_bytes(npairs, w, h, stride) if work_bytes is None else work_bytes
    return capi.lib().ofdis_dense_tracks(_p(hb.frames, frames), _p(hb.flow, fw), _p(hb.flow, rev), npairs, w, h, noc, stride, window,
                                         min_eig, max_len, alpha, beta, max_tracks, _p(hb.tracks, tracks), _p(hb.start, start),
                                         _p(hb.len, length), _p(hb.info, info), hb.work.ctypes.data + work_offset if work else None,
                                         wb, None)


def _texture(hb, frames=True, out=True, nframes=3, w=16, h=8, noc=1, stride=4, window=1, min_eig=5):
    return capi.lib().ofdis_seed_texture(_p(hb.frames, frames), nframes, w, h, noc, stride, window, min_eig, _p(hb.out, out), None)


@pytest.mark.parametrize("which", ["frames", "fw", "tracks", "start", "info", "work"])
def test_rejects_null_pointers(which):
    abi.rejected(_dense(_Host(), **{which: False}), "flow_fw" if which == "fw" else which)


@pytest.mark.parametrize("which", ["frames", "out"])
def test_seed_texture_rejects_null_pointers(which):
    abi.rejected(_texture(_Host(), **{which: False}), which)


@pytest.mark.parametrize("call", [_dense, _texture])
@pytest.mark.parametrize("kw,word", [
    (dict(noc=0), "noc"), (dict(noc=2), "noc"), (dict(noc=4), "noc"), (dict(noc=-1), "noc"),
    (dict(stride=1), "stride"), (dict(stride=0), "stride"), (dict(stride=-4), "stride"), (dict(stride=65), "stride"),
    (dict(window=-1), "window"), (dict(window=8), "window"), (dict(min_eig=-1), "min_eig"),
    (dict(stride=9), "stride"), (dict(w=3), "stride"), (dict(stride=64, w=64, h=63), "stride"),
    (dict(w=0), "size"), (dict(h=0), "size"), (dict(w=-16), "size"), (dict(w=1 << 16, h=1 << 16), "size"),
], ids=lambda v: ",".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else "")
def test_rejects_what_both_calls_check(call, kw, word):
    abi.rejected(call(_Host(), **kw), word)


@pytest.mark.parametrize("kw,word", [
    (dict(max_len=-1), "max_len"), (dict(max_tracks=0), "max_tracks"), (dict(max_tracks=-1), "max_tracks"),
    (dict(max_tracks=(1 << 24) + 1), "max_tracks"), (dict(npairs=0), "npairs"), (dict(npairs=-1), "npairs"),
    (dict(alpha=-0.01), "alpha"), (dict(beta=-0.5), "alpha"), (dict(alpha=math.nan), "alpha"), (dict(beta=math.inf), "alpha"),
    (dict(work_bytes=0), "work"), (dict(work_offset=4), "work"), (dict(work_offset=1), "work"),
], ids=lambda v: ",".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else "")
def test_rejects(kw, word):
    abi.rejected(_dense(_Host(), **kw), word)


@pytest.mark.parametrize("nframes", [0, -1])
def test_seed_texture_rejects_nframes(nframes):
    abi.rejected(_texture(_Host(), nframes=nframes), "nframes")


def test_a_work_buffer_one_byte_short_is_rejected():
    wb = capi.lib().ofdis_dense_tracks_work_bytes(2, 16, 8, 4)
    assert 0 < wb <= 1 << 16
    abi.rejected(_dense(_Host(), work_bytes=wb - 1), "work")


def test_the_value_checks_accept_their_closed_ranges():
    """both ends of every range, max_tracks = 2^24 among them: the call passes that check and fails at the next one (the
    sizes, and behind them the work buffer)"""
    hb = _Host()
    for kw in (dict(max_tracks=1 << 24), dict(max_tracks=1), dict(stride=2), dict(stride=64), dict(window=0), dict(window=7),
               dict(min_eig=0), dict(min_eig=2 ** 31 - 1), dict(max_len=0), dict(max_len=2 ** 31 - 1), dict(alpha=0.0, beta=0.0),
               dict(noc=3), dict(rev=False), dict(length=False)):
        abi.rejected(_dense(hb, **dict(dict(w=0), **kw)), "size")
    for kw in (dict(max_tracks=1 << 24), dict(max_len=2 ** 31 - 1), dict(rev=False), dict(length=False)):
        abi.rejected(_dense(hb, work_bytes=8, **kw), "work")


def test_batch_form_without_a_context():
    hb = _Host()
    rc = capi.lib().ofdis_batch_dense_tracks(None, hb.frames.ctypes.data, 0, 2, 4, 1, 5, 0, 1, capi.FB_ALPHA, capi.FB_BETA, 64,
                                             hb.tracks.ctypes.data, hb.start.ctypes.data, None, hb.info.ctypes.data, 16, 8, None)
    abi.rejected(rc, "SEQUENCE")
