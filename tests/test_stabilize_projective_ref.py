"""CPU: the numpy model of the projective stabiliser (of_dis_amd/stabilize.py: camera_path_projective_ref, warp_positions8,
warp_frames_projective_ref), the definition the kernels are compared with in tests/test_gpu_stabilize_projective.py -- the
consequences include/ofdis.h states, on inputs whose answer is known, and the preconditions of the end-to-end test."""
import math

import numpy as np
import pytest

import stab_projective as sp
from of_dis_amd import gmotion, stabilize
from of_dis_amd.stabilize import (BORDER_CONSTANT, BORDER_REPLICATE, camera_path_projective_ref, camera_path_ref, compose8,
                                  gaussian_weights, invert8, smoothed_map8, warp_frames_projective_ref, warp_frames_ref,
                                  warp_positions, warp_positions8)
from test_stabilize_ref import frames_of, rotations

SIZES = [(64, 16), (37, 11), (6, 5), (1, 1)]


def bits(a):
    return np.ascontiguousarray(a).view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def widened(m6, a6=0.0, a7=0.0):
    m = np.zeros((len(m6), 8))
    m[:, :6], m[:, 6], m[:, 7] = m6, a6, a7
    return m


# ------------------------------------------------------------------ the frame warp
@pytest.mark.parametrize("w,h", SIZES)
def test_without_perspective_terms_the_positions_are_the_affine_ones(w, h):
    rng = np.random.default_rng(w + h)
    for _ in range(50):
        b = rng.normal(0, 1, 6) * np.array([2, .05, .05, 2, .05, .05])
        px, py, front = warp_positions8(np.r_[b, 0.0, 0.0], w, h)
        ax, ay = warp_positions(b, w, h)
        assert np.array_equal(bits(px), bits(ax)) and np.array_equal(bits(py), bits(ay)) and front.all()
        px, py, front = warp_positions8(np.r_[b, -0.0, -0.0], w, h)      # (e = -0 or +0: D = 1 either way)
        assert np.array_equal(px, ax) and np.array_equal(py, ay) and front.all()


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("border", [BORDER_CONSTANT, BORDER_REPLICATE])
def test_without_perspective_terms_the_frames_are_the_affine_ones(noc, border):
    for w, h in SIZES:
        fr = frames_of(4, w, h, noc)
        b = np.random.default_rng(5).normal(0, 1, (4, 6)) * np.array([2, .05, .05, 2, .05, .05])
        b[0] = 0.0
        got, want = warp_frames_projective_ref(fr, widened(b), border), warp_frames_ref(fr, b, border)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[0][0], fr[0]) and (got[1][0] == 1).all()           # a zero warp returns the frame


@pytest.mark.parametrize("noc", [1, 3])
def test_an_integer_translation_shifts_the_frame(noc):
    w, h = 21, 9
    fr = frames_of(2, w, h, noc)
    warps = np.zeros((2, 8))
    warps[:, 0], warps[:, 3] = 3.0, -2.0
    out, ins = warp_frames_projective_ref(fr, warps, BORDER_CONSTANT)
    assert np.array_equal(out[:, 2:, :w - 3], fr[:, :h - 2, 3:])
    assert not out[:, :2].any() and not out[:, :, w - 3:].any()
    assert ins[:, 2:, :w - 3].all() and ins.sum() == 2 * (h - 2) * (w - 3)


def test_positions_follow_the_homography():
    """against gmotion.homography in float64 at 256 x 128 with perspective terms up to 3e-4: within 1e-3 px (the positions are
    fp32: an ulp of 255 is 1.5e-5, and the displacement form keeps the rounding of mu, r and their product at that size)"""
    w, h = 256, 128
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    xc, yc = xs - (w - 1) / 2, ys - (h - 1) / 2
    rng = np.random.default_rng(9)
    worst = 0.0
    for k in range(20):
        g = rng.normal(0, 1, 8) * np.array([2, .02, .02, 2, .02, .02, 0, 0])
        g[6:] = rng.uniform(-3e-4, 3e-4, 2) if k else (3e-4, -3e-4)
        H = gmotion.homography(g)
        den = H[2, 0] * xc + H[2, 1] * yc + H[2, 2]
        ex = (H[0, 0] * xc + H[0, 1] * yc + H[0, 2]) / den + (w - 1) / 2
        ey = (H[1, 0] * xc + H[1, 1] * yc + H[1, 2]) / den + (h - 1) / 2
        px, py, front = warp_positions8(g, w, h)
        assert front.all()
        worst = max(worst, np.abs(px - ex).max(), np.abs(py - ey).max())
    assert worst < 1e-3, worst


def test_behind_the_camera_is_outside():
    """g6 = 4 / W: the denominator crosses zero inside the frame; inside is 0 wherever D <= 0 and on part of the rest"""
    w, h = 64, 16
    g = np.zeros((1, 8))
    g[0, 6] = 4.0 / w
    px, py, front = warp_positions8(g[0], w, h)
    assert front[:, :w // 4 + 8].all() and not front[:, 3 * w // 4:].any() and 0 < front.sum() < w * h
    out, ins = warp_frames_projective_ref(frames_of(1, w, h, 1), g, BORDER_CONSTANT)
    assert not ins[0][~front].any() and not out[0][~front].any() and 0 < ins.sum() < front.sum()
    for bad in (math.nan, math.inf, -math.inf):
        g[0, 6] = bad
        assert not warp_frames_projective_ref(frames_of(1, w, h, 1), g, BORDER_CONSTANT)[1].any()


def test_the_border_mode_is_checked():
    with pytest.raises(ValueError):
        warp_frames_projective_ref(frames_of(1, 4, 4, 1), np.zeros((1, 8)), 2)


# ------------------------------------------------------------------ the camera path
def test_affine_models_give_the_affine_path_to_rounding():
    """a6 = a7 = 0: g6 = g7 = 0 exactly, and g0 .. g5 within 1e-12 * max(1, |warp|) of ofdis_camera_path's (the translation of the
    inverse is rounded differently; a few hundred fp64 operations on values of that size accumulate about a hundredth of it)"""
    rng = np.random.default_rng(0)
    m = rng.normal(0, 1, (300, 6)) * np.array([3, .02, .02, 3, .02, .02])
    for radius in (1, 3, 64):
        wt = gaussian_weights(radius, max(radius / 3.0, 0.5))
        for zoom in (1.0, 1.25):
            a = camera_path_ref(m, wt, zoom)
            p = camera_path_projective_ref(widened(m), wt, zoom, 256, 128)
            assert not bits(np.ascontiguousarray(p[:, 6:])).any()                    # +0, not -0
            assert (np.abs(p[:, :6] - a) <= 1e-12 * np.maximum(1.0, np.abs(a))).all(), np.abs(p[:, :6] - a).max()
    assert np.abs(a).max() > 5.0


def test_zero_models_radius_zero_and_the_ends_give_the_identity():
    w = gaussian_weights(5, 2.0)
    m = widened(rotations(9), 1e-4, -2e-4)
    assert not bits(camera_path_projective_ref(np.zeros((9, 8)), w, 1.0, 256, 128)).any()
    assert not bits(camera_path_projective_ref(m, [1.0], 1.0, 256, 128)).any()
    p = camera_path_projective_ref(m, w, 1.0, 256, 128)
    assert p.shape == (10, 8) and not bits(p[0]).any() and not bits(p[-1]).any()      # the clip's ends: reach 0
    assert np.abs(p[1:-1, 6:]).min() > 0 and np.abs(p[1:-1]).max() > 1e-3


def test_windows_are_truncated_symmetrically():
    m = widened(rotations(30, seed=5, angle=0.02), -1e-4, 5e-5)
    w = gaussian_weights(6, 3.0)
    hx, hy = stabilize.half_sides(256, 128)
    assert [smoothed_map8(m, f, w, hx, hy)[1] for f in range(31)] == [min(6, f, 30 - f) for f in range(31)]


def test_the_warp_inverts_the_smoothed_map():
    m = widened(rotations(30, seed=5, angle=0.02), -1e-4, 5e-5)
    w = gaussian_weights(6, 3.0)
    hx, hy = stabilize.half_sides(256, 128)
    warps = camera_path_projective_ref(m, w, 1.0, 256, 128)
    for f in range(31):
        Q = smoothed_map8(m, f, w, hx, hy)[0]
        g = warps[f]
        W = (1.0 + g[1], g[2], g[4], 1.0 + g[5], g[0], g[3], 0.0 - g[6], 0.0 - g[7])
        assert np.abs(np.array(compose8(W, Q)) - np.array(stabilize.IDENTITY8)).max() < 1e-12, f
        assert np.abs(np.array(compose8(Q, invert8(Q))) - np.array(stabilize.IDENTITY8)).max() < 1e-12, f


def test_compose_is_the_matrix_product():
    rng = np.random.default_rng(4)
    for _ in range(20):
        a, b = (rng.normal(0, 1, 8) * np.array([3, .02, .02, 3, .02, .02, 1e-3, 1e-3]) for _ in range(2))
        Ta, Tb = (stabilize.pair_map8(x, 0.0, 0.0)[0] for x in (a, b))
        H = gmotion.homography(a) @ gmotion.homography(b)
        assert np.abs(sp.model_of(H) - sp.model_of(_matrix(compose8(Ta, Tb)))).max() < 1e-12
        assert np.abs(sp.model_of(np.linalg.inv(gmotion.homography(a))) - sp.model_of(_matrix(invert8(Ta)))).max() < 1e-12


def _matrix(T):
    return np.array([[T[0], T[1], T[4]], [T[2], T[3], T[5]], [T[6], T[7], 1.0]])


@pytest.mark.parametrize("kind", ["nan", "inf", "det0", "denominator", "nan-a7"])
def test_an_unusable_pair_splits_the_clip(kind):
    m = widened(rotations(15, seed=8), 1e-4, 1e-4)
    k = 7
    if kind == "nan":
        m[k, 3] = math.nan
    elif kind == "inf":
        m[k, 6] = math.inf
    elif kind == "det0":
        m[k, [1, 2, 4, 5]] = -1.0, 0.0, 0.0, 0.0
    elif kind == "denominator":
        m[k, 6] = 0.004                                       # 127.5 * 0.004 = 0.51
    else:
        m[k, 7] = math.nan
    w = gaussian_weights(6, 3.0)
    for zoom in (1.0, 1.25):
        whole = camera_path_projective_ref(m, w, zoom, 256, 128)
        halves = np.concatenate([camera_path_projective_ref(m[:k], w, zoom, 256, 128),
                                 camera_path_projective_ref(m[k + 1:], w, zoom, 256, 128)])
        assert np.array_equal(bits(whole), bits(halves)) and np.isfinite(whole).all()
        assert np.abs(whole[[2, 3, 11, 12]]).max() > 1e-3
    if kind == "denominator":                                 # the bound looks at the frame: a 1 x 1 frame has none
        assert smoothed_map8(m, k, w, 0.0, 0.0)[1] == 6


def test_the_denominator_bound_is_inclusive():
    """W = 257: hx = 128, so a6 = -2^-8 gives 1 - |gx| * hx = 0.5 exactly: usable; one ulp more is a break.  Likewise in y."""
    for col, (w, h) in ((6, (257, 1)), (7, (1, 257))):
        for a, usable in ((2.0 ** -8, True), (-2.0 ** -8, True), (2.0 ** -8 + 2.0 ** -60, False), (-2.0 ** -8 - 2.0 ** -60, False)):
            m = widened(rotations(3, seed=1))
            m[1, col] = a
            hx, hy = stabilize.half_sides(w, h)
            assert (1.0 - abs(a) * 128.0 == 0.5) == usable
            assert (smoothed_map8(m, 1, [1.0, 1.0], hx, hy)[1] == 1) == usable, (col, a)
            assert smoothed_map8(m, 1, [1.0, 1.0], 0.0, 0.0)[1] == 1
    # both terms together: 0.25 + 0.25 is at the bound, and it is the sum that counts
    m = widened(rotations(3, seed=1), 2.0 ** -9, -2.0 ** -9)
    assert smoothed_map8(m, 1, [1.0, 1.0], 128.0, 128.0)[1] == 1
    m[1, 7] = -2.0 ** -9 - 2.0 ** -60
    assert smoothed_map8(m, 1, [1.0, 1.0], 128.0, 128.0)[1] == 0


def test_huge_finite_models_end_in_the_identity():
    m = widened(rotations(6, seed=2), 1e-4, 0.0)
    m[2, 0], m[3, 3] = 1.7e308, -1.7e308
    warps = camera_path_projective_ref(m, gaussian_weights(3, 2.0), 1.25, 256, 128)
    assert np.isfinite(warps).all()
    assert np.array_equal(bits(warps[3]), bits(np.array([0.0, 0.8 - 1.0, 0.0, 0.0, 0.0, 0.8 - 1.0, 0.0, 0.0])))


def test_zoom_scales_about_the_centre():
    warps = camera_path_projective_ref(np.zeros((4, 8)), gaussian_weights(3, 1.5), 2.0, 64, 16)
    assert np.array_equal(bits(warps), bits(np.tile([0.0, -0.5, 0.0, 0.0, 0.0, -0.5, 0.0, 0.0], (5, 1))))


@pytest.mark.parametrize("weights,zoom,w,h", [([], 1.0, 8, 8), ([0.0, 1.0], 1.0, 8, 8), ([1.0, math.nan], 1.0, 8, 8),
                                              ([1.0] * 66, 1.0, 8, 8), ([1.0], 0.99, 8, 8), ([1.0], 16.5, 8, 8),
                                              ([1.0], 1.0, 0, 8), ([1.0], 1.0, 8, 0), ([1.0], 1.0, 8193, 8), ([1.0], 1.0, 8, 8193)])
def test_the_window_and_size_checks(weights, zoom, w, h):
    with pytest.raises(ValueError):
        camera_path_projective_ref(np.zeros((2, 8)), weights, zoom, w, h)


def test_the_generated_models_meet_their_conditions():
    """what tests/test_gpu_stabilize_projective.py relies on, checked here where no device is needed"""
    w = gaussian_weights(64, 20.0)
    smooth, wild = sp.models8(300, "smooth"), sp.models8(300, "wild")
    reach = sp.reach8(smooth, w, 256, 128)
    assert reach.max() == 64 and (reach == 64).sum() == 301 - 128
    path = camera_path_projective_ref(smooth, w, 1.0, 256, 128)
    assert np.abs(path[:, :6]).max() > 1.0 and np.abs(path[:, 6:]).max() > 1e-6
    reach = sp.reach8(wild, w, 256, 128)
    assert (reach == 0).sum() > 30 and 3 < reach.max() < 64
    assert (sp.reach8(wild, w, 1, 1) != reach).any()           # some breaks are the denominator bound's alone
    assert np.isfinite(camera_path_projective_ref(wild, w, 1.25, 256, 128)).all()


# ------------------------------------------------------------------ the end-to-end clip: its preconditions
E2E = dict(w=256, h=128, n=25, fl=150.0, pan_deg=0.5, jitter_deg=(1.0, 1.0, 0.5), seed=1)


def e2e_ideals(w, h, n, fl, pan_deg, jitter_deg, seed):
    """(C, true models, the projective share with the true models, the affine share with their least-squares affine parts)"""
    C = sp.camera_homographies(n, fl, pan_deg, jitter_deg, seed)
    true = sp.true_models(C)
    weights = gaussian_weights(4, 2.0)
    proj = sp.corner_share(camera_path_projective_ref(true, weights, 1.0, w, h), C, w, h)
    aff6 = np.array([sp.affine_part(C[f + 1] @ np.linalg.inv(C[f]), w, h) for f in range(n - 1)])
    aff = sp.corner_share(camera_path_ref(aff6, weights, 1.0), C, w, h)
    return C, true, proj, aff


def test_the_end_to_end_clip_separates_the_two_paths():
    """the true models of the rotating camera: every pair usable, the projective path leaves less than 0.15 of the corners'
    roughness (0.093), the affine path fed the least-squares affine parts more than 0.30 (0.373)"""
    C, true, proj, aff = e2e_ideals(**E2E)
    hx, hy = stabilize.half_sides(E2E["w"], E2E["h"])
    assert all(stabilize.pair_map8(m, hx, hy)[1] for m in true)
    assert np.abs(true[:, 6:]).max() > 1e-4
    assert proj < 0.15 and aff > 0.30, (proj, aff)
    assert abs(proj - 0.093) < 2e-3 and abs(aff - 0.373) < 2e-3, (proj, aff)
