"""CPU: argument checks of the point-trajectory entry points (include/ofdis.h: ofdis_track_points, ofdis_batch_track_points)
that return before any device work, and properties of the numpy statement of the definition (of_dis_amd/tracking.py).  Host
buffers stand in for the device arrays: every call here returns before it would launch.  The kernels, and the checks that
need a context (creating one needs a device): tests/test_gpu_track.py."""
import math

import numpy as np
import pytest

import abi
from of_dis_amd import capi, tracking
from stereo_lr_ref import bits as _bits

_f32 = np.float32


def test_max_points_matches_the_header():
    assert abi.define("OFDIS_TRACK_MAX_POINTS") == capi.TRACK_MAX_POINTS


def test_defaults_match_the_binding():
    assert (tracking.FB_ALPHA, tracking.FB_BETA) == (capi.FB_ALPHA, capi.FB_BETA)


class _Host:
    """host stand-ins for a 2-pair 8x4 case of 3 points"""

    def __init__(self, w=8, h=4, npairs=2, n=3):
        self.flow = np.zeros((npairs, h, w, 2), _f32)
        self.seeds = np.zeros((n, 2), _f32)
        self.seed_frame = np.zeros(n, np.int32)
        self.tracks = np.zeros((npairs + 1, n, 2), _f32)
        self.counts = np.zeros(n, np.int32)


def _track(hb, fw=True, rev=True, seeds=True, tracks=True, npairs=2, w=8, h=4, npoints=3, max_steps=0, alpha=capi.FB_ALPHA,
           beta=capi.FB_BETA):
    p = abi.ptr
    return capi.lib().ofdis_track_points(p(hb.flow, fw), p(hb.flow, rev), npairs, w, h, p(hb.seeds, seeds),
                                         hb.seed_frame.ctypes.data, npoints, max_steps, alpha, beta, p(hb.tracks, tracks),
                                         hb.counts.ctypes.data, None)


@pytest.mark.parametrize("which", ["fw", "seeds", "tracks"])
def test_track_points_rejects_null_pointers(which):
    abi.rejected(_track(_Host(), **{which: False}))


@pytest.mark.parametrize("npoints", [0, -1, (1 << 24) + 1])
def test_track_points_rejects_npoints(npoints):
    abi.rejected(_track(_Host(), npoints=npoints))
    assert "npoints" in capi.lib().ofdis_last_error().decode()


def test_track_points_rejects_negative_max_steps():
    abi.rejected(_track(_Host(), max_steps=-1))
    assert "max_steps" in capi.lib().ofdis_last_error().decode()


@pytest.mark.parametrize("npairs,w,h", [(0, 8, 4), (-1, 8, 4), (2, 0, 4), (2, 8, 0), (2, -8, 4), (2, 1 << 16, 1 << 16)])
def test_track_points_rejects_bad_sizes(npairs, w, h):
    abi.rejected(_track(_Host(), npairs=npairs, w=w, h=h))
    assert "size" in capi.lib().ofdis_last_error().decode()


@pytest.mark.parametrize("kw", [dict(alpha=-0.01), dict(beta=-0.5), dict(alpha=math.nan), dict(beta=math.inf),
                                dict(alpha=math.inf), dict(beta=math.nan)], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_track_points_rejects_alpha_beta(kw):
    """as ofdis_fb_check rejects them, with and without the reverse flow"""
    abi.rejected(_track(_Host(), **kw))
    abi.rejected(_track(_Host(), rev=False, **kw))


def test_track_points_checks_pass_the_largest_point_count():
    """npoints = OFDIS_TRACK_MAX_POINTS passes the point-count check: the call gets as far as the size check"""
    abi.rejected(_track(_Host(), npoints=capi.TRACK_MAX_POINTS, npairs=0))
    assert "size" in capi.lib().ofdis_last_error().decode()


def test_batch_track_points_without_a_context():
    hb = _Host()
    rc = capi.lib().ofdis_batch_track_points(None, 0, 2, hb.seeds.ctypes.data, None, 3, 0, 1, capi.FB_ALPHA, capi.FB_BETA,
                                             hb.tracks.ctypes.data, None, 8, 4, None)
    abi.rejected(rc)


# ------------------------------------------------------------------ the numpy statement of the definition
@pytest.mark.parametrize("d", [(0.25, -0.5), (1.75, 0.25), (-2.5, 1.0), (0.0, 0.0)])
def test_constant_flow_moves_a_seed_by_k_times_d(d):
    """quarter-pixel values: every position and every product of the bilinear blend is exact in float32"""
    w, h, npairs = 40, 30, 6
    fw = np.broadcast_to(np.array(d, _f32), (npairs, h, w, 2)).copy()
    seeds = np.array([[20.0, 15.0], [19.25, 14.5], [20.5, 15.75]], _f32)
    for rev in (-fw, None):
        tracks, counts = tracking.track_ref(fw, rev, seeds)
        assert counts.tolist() == [npairs + 1] * 3
        for k in range(npairs + 1):
            want = seeds + _f32(k) * np.array(d, _f32)
            assert np.array_equal(_bits(tracks[k]), _bits(want)), (d, k)


def test_max_steps_bounds_the_count():
    w, h, npairs = 16, 12, 5
    fw = np.zeros((npairs, h, w, 2), _f32)
    seeds = tracking.grid_seeds(w, h, 3)
    sf = np.arange(seeds.shape[0], dtype=np.int32) % (npairs + 1)
    tracks, counts = tracking.track_ref(fw, -fw, seeds, sf, max_steps=1)
    assert counts.max() == 2 and (counts <= 2).all()
    assert (counts[sf == npairs] == 1).all() and (counts[sf < npairs] == 2).all()
    tracks, counts = tracking.track_ref(fw, -fw, seeds, sf, max_steps=3)
    assert np.array_equal(counts, np.minimum(3, npairs - sf) + 1)


def test_a_seed_at_the_last_frame_has_one_entry():
    w, h, npairs = 9, 7, 3
    fw = np.full((npairs, h, w, 2), 100.0, _f32)  # (never sampled)
    seeds = np.array([[4.5, 3.25]], _f32)
    tracks, counts = tracking.track_ref(fw, None, seeds, np.array([npairs]))
    assert counts.tolist() == [1]
    assert np.array_equal(_bits(tracks[npairs, 0]), _bits(seeds[0]))
    assert (_bits(tracks[:npairs]) == tracking.ENDED_BITS).all()
    assert tracking.ended(tracks)[:, 0].tolist() == [True] * npairs + [False]


def test_seeds_that_start_no_track():
    """outside the image, NaN, a seed frame out of range: count 0 and the NaN pattern everywhere"""
    w, h, npairs = 9, 7, 2
    fw = np.zeros((npairs, h, w, 2), _f32)
    seeds = np.array([[-0.25, 3], [8.5, 3], [4, 6.001], [np.nan, 2], [4, 3], [4, 3], [8, 6], [0, 0]], _f32)
    sf = np.array([0, 0, 0, 0, -1, npairs + 1, 0, 0])
    tracks, counts = tracking.track_ref(fw, -fw, seeds, sf)
    assert counts.tolist() == [0, 0, 0, 0, 0, 0, npairs + 1, npairs + 1]
    assert (_bits(tracks[:, :6]) == tracking.ENDED_BITS).all()
    assert not tracking.ended(tracks[:, 6:]).any()


def test_a_track_ends_where_it_leaves_the_image_or_fails_the_test():
    w, h, npairs = 20, 10, 4
    fw = np.zeros((npairs, h, w, 2), _f32)
    fw[..., 0] = 6.0
    rev = -fw
    rev[2] = 0.0  # pair 2: the reverse flow does not lead back (lhs = 36 > 0.01 * 36 + 0.5)
    why = {}
    tracks, counts = tracking.track_ref(fw, rev, np.array([[1, 5], [9, 5]], _f32), reasons=why)
    assert counts.tolist() == [3, 2]  # 1 -> 7 -> 13 -> inconsistent;  9 -> 15 -> 21 is outside
    assert why == {"outside": 1, "inconsistent": 1}
    assert tracks[2, 0].tolist() == [13.0, 5.0] and tracking.ended(tracks[3:, 0]).all()
