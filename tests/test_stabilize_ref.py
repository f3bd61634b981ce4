"""CPU: the numpy model of the video stabilisation (of_dis_amd/stabilize.py: camera_path_ref, warp_frames_ref), the definition
the kernels are compared with in tests/test_gpu_stabilize.py -- its properties on inputs whose answer is known."""
import math

import numpy as np
import pytest

from of_dis_amd import stabilize
from of_dis_amd.stabilize import (BORDER_CONSTANT, BORDER_REPLICATE, camera_path_ref, compose, gaussian_weights, smoothed_map,
                                  warp_frames_ref)

_f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view({1: np.uint8, 8: np.uint64}[a.dtype.itemsize])


def rotations(n, seed=3, angle=0.01, shift=2.0):
    """n models that are small rotations (up to `angle` rad) with translations up to `shift` px"""
    rng = np.random.default_rng(seed)
    m = np.zeros((n, 6))
    th = rng.uniform(-angle, angle, n)
    m[:, 1], m[:, 2], m[:, 4], m[:, 5] = np.cos(th) - 1, -np.sin(th), np.sin(th), np.cos(th) - 1
    m[:, 0], m[:, 3] = rng.uniform(-shift, shift, n), rng.uniform(-shift, shift, n)
    return m


# ------------------------------------------------------------------ camera path
def test_zero_models_and_radius_zero_give_zero_warps():
    w = gaussian_weights(5, 2.0)
    assert not bits(camera_path_ref(np.zeros((9, 6)), w)).any()          # (all-zero bits: no negative zero either)
    assert not bits(camera_path_ref(rotations(9), [1.0])).any()
    assert not bits(camera_path_ref(rotations(9), [0.3])).any()
    assert camera_path_ref(np.zeros((1, 6)), w).shape == (2, 6)


def test_a_uniform_pan_is_left_alone():
    m = np.zeros((20, 6))
    m[:, 0], m[:, 3] = 2.0, -1.0
    for radius, sigma in ((4, 2.0), (8, 3.0), (30, 10.0)):
        warps = camera_path_ref(m, gaussian_weights(radius, sigma))
        assert np.abs(warps[:, [0, 3]]).max() < 1e-12
        assert not bits(warps[0]).any() and not bits(warps[-1]).any()
        assert np.abs(warps).max() < 1e-12


@pytest.mark.parametrize("kind", ["nan", "inf", "det0", "det5", "det-negative"])
def test_an_unusable_pair_splits_the_clip(kind):
    m = rotations(15, seed=8)
    k = 7
    if kind == "nan":
        m[k, 3] = math.nan
    elif kind == "inf":
        m[k, 0] = math.inf
    elif kind == "det0":
        m[k, [1, 2, 4, 5]] = -1.0, 0.0, 0.0, 0.0            # A = [[0, 0], [0, 1]]
    elif kind == "det5":
        m[k, [1, 2, 4, 5]] = 4.0, 0.0, 0.0, 0.0             # A = [[5, 0], [0, 1]]
    else:
        m[k, [1, 2, 4, 5]] = -2.0, 0.0, 0.0, 0.0            # a mirror
    w = gaussian_weights(6, 3.0)
    for zoom in (1.0, 1.25):
        whole = camera_path_ref(m, w, zoom)
        halves = np.concatenate([camera_path_ref(m[:k], w, zoom), camera_path_ref(m[k + 1:], w, zoom)])
        assert np.array_equal(bits(whole), bits(halves))
        assert np.abs(whole[[2, 3, 11, 12]]).max() > 1e-3       # (the halves are really smoothed)
    assert smoothed_map(m, k, w)[1] == 0 and smoothed_map(m, k + 1, w)[1] == 0
    assert smoothed_map(m, k - 2, w)[1] == 2 and smoothed_map(m, k + 4, w)[1] == 3


def test_the_determinant_limits_are_inclusive():
    """A = [[1, 1], [c, 1]] has det = 1 - c, exact for the four values of c below"""
    for c, det, usable in ((0.75, 0.25, True), (-3.0, 4.0, True), (0.75 + 2.0 ** -53, 0.25 - 2.0 ** -53, False),
                           (-3.0 - 2.0 ** -50, 4.0 + 2.0 ** -50, False)):
        assert 1.0 - c == det and (det in (0.25, 4.0)) == usable
        m = rotations(3, seed=1)
        m[1, [1, 2, 4, 5]] = 0.0, 1.0, c, 0.0
        assert (smoothed_map(m, 1, [1.0, 1.0])[1] == 1) == usable, det


def test_zoom_scales_about_the_centre():
    warps = camera_path_ref(np.zeros((4, 6)), gaussian_weights(3, 1.5), zoom=2.0)
    assert np.array_equal(bits(warps), bits(np.tile([0.0, -0.5, 0.0, 0.0, 0.0, -0.5], (5, 1))))


def test_the_warp_inverts_the_smoothed_map():
    m = rotations(30, seed=5, angle=0.02)
    w = gaussian_weights(6, 3.0)
    warps = camera_path_ref(m, w)
    reached = 0
    for f in range(31):
        Q, r = smoothed_map(m, f, w)
        b = warps[f]
        W = (1.0 + b[1], b[2], b[4], 1.0 + b[5], b[0], b[3])
        assert np.abs(np.array(compose(W, Q)) - np.array(stabilize.IDENTITY)).max() < 1e-12, f
        assert r == min(6, f, 30 - f)
        reached += r == 6
    assert reached == 19


def test_huge_finite_models_end_in_the_identity():
    """a usable pair whose translation overflows the chain: the warp is the identity, never a NaN or an infinity"""
    m = rotations(6, seed=2)
    m[2, 0], m[3, 3] = 1.7e308, -1.7e308
    warps = camera_path_ref(m, gaussian_weights(3, 2.0), 1.25)
    assert np.isfinite(warps).all()
    assert np.array_equal(bits(warps[3]), bits(np.array([0.0, 0.8 - 1.0, 0.0, 0.0, 0.0, 0.8 - 1.0])))


@pytest.mark.parametrize("weights,zoom", [([], 1.0), ([0.0, 1.0], 1.0), ([1.0, -0.1], 1.0), ([1.0, math.nan], 1.0),
                                          ([1.0, math.inf], 1.0), ([1.0] * 66, 1.0), ([1.0], 0.99), ([1.0], 16.5),
                                          ([1.0], math.nan), ([1.0], math.inf)])
def test_the_window_checks(weights, zoom):
    with pytest.raises(ValueError):
        camera_path_ref(np.zeros((2, 6)), weights, zoom)


def test_gaussian_weights():
    w = gaussian_weights(4, 2.0)
    assert w.dtype == np.float64 and w.shape == (5,) and w[0] == 1.0 and (np.diff(w) < 0).all()
    assert w[2] == math.exp(-0.5)
    assert gaussian_weights(0, 1.0).tolist() == [1.0]
    for bad in ((-1, 1.0), (65, 1.0), (3, 0.0), (3, math.nan)):
        with pytest.raises(ValueError):
            gaussian_weights(*bad)


# ------------------------------------------------------------------ frame warp
def frames_of(n, w, h, noc, seed=11):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w) + ((3,) if noc == 3 else ()), dtype=np.uint8)


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("border", [BORDER_CONSTANT, BORDER_REPLICATE])
def test_a_zero_warp_returns_the_frames(noc, border):
    for w, h in ((37, 11), (1, 1), (1, 7), (9, 1)):
        fr = frames_of(3, w, h, noc)
        out, ins = warp_frames_ref(fr, np.zeros((3, 6)), border)
        assert out.dtype == np.uint8 and np.array_equal(out, fr) and (ins == 1).all()


@pytest.mark.parametrize("noc", [1, 3])
def test_an_integer_translation_shifts_the_frame(noc):
    w, h = 21, 9
    fr = frames_of(2, w, h, noc)
    warps = np.zeros((2, 6))
    warps[:, 0], warps[:, 3] = 3.0, -2.0                      # out(x, y) = I(x + 3, y - 2)
    out, ins = warp_frames_ref(fr, warps, BORDER_CONSTANT)
    assert np.array_equal(out[:, 2:, :w - 3], fr[:, :h - 2, 3:])
    assert not out[:, :2].any() and not out[:, :, w - 3:].any()
    want = np.zeros((h, w), np.uint8)
    want[2:, :w - 3] = 1
    assert np.array_equal(ins, np.stack([want, want]))
    rep, ins_r = warp_frames_ref(fr, warps, BORDER_REPLICATE)
    assert np.array_equal(ins_r, ins)
    assert np.array_equal(rep[:, 2:, :w - 3], fr[:, :h - 2, 3:])
    ys, xs = np.clip(np.arange(h) - 2, 0, h - 1), np.clip(np.arange(w) + 3, 0, w - 1)
    assert np.array_equal(rep, fr[:, ys][:, :, xs])           # the uncovered rows and columns repeat the edge


@pytest.mark.parametrize("noc", [1, 3])
def test_a_nan_warp_is_outside_everywhere(noc):
    fr = frames_of(2, 13, 6, noc)
    warps = np.zeros((2, 6))
    warps[0, 0], warps[1, 5] = math.nan, math.nan
    out, ins = warp_frames_ref(fr, warps, BORDER_CONSTANT)
    assert not ins.any() and not out.any()
    out, ins = warp_frames_ref(fr, warps, BORDER_REPLICATE)
    assert not ins.any()
    assert (out[0] == fr[0][:, :1]).all()                     # x is NaN: column 0 of every row
    assert (out[1] == fr[1][:1]).all()                        # y is NaN: row 0 of every column


def test_a_half_pixel_shift_averages_neighbours():
    fr = frames_of(1, 8, 4, 1)
    warps = np.zeros((1, 6))
    warps[0, 0] = 0.5
    out, ins = warp_frames_ref(fr, warps, BORDER_REPLICATE)
    a, b = fr[0, :, :-1].astype(np.int64), fr[0, :, 1:].astype(np.int64)
    assert np.array_equal(out[0, :, :-1], (a + b + 1) // 2)   # floor((a + b) / 2 + 0.5)
    assert np.array_equal(out[0, :, -1], fr[0, :, -1]) and (ins[0, :, :-1] == 1).all() and not ins[0, :, -1].any()


def test_the_border_mode_is_checked():
    with pytest.raises(ValueError):
        warp_frames_ref(frames_of(1, 4, 4, 1), np.zeros((1, 6)), 2)
