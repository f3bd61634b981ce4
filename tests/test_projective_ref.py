"""CPU: the numpy model of the 8-parameter projective camera models (of_dis_amd/gmotion.py: sums23, solve8,
projective_motion_ref, projective_compensate_ref, model_flow8, homography -- the definition of include/ofdis.h, "Projective camera
models") on its own: the sums, the solve and its rank test, the fallbacks, and what the model buys on a true camera pan.  The
kernels are held to this model bit for bit in tests/test_gpu_projective.py."""
import numpy as np
import pytest

from of_dis_amd import gmotion, tracking
from of_dis_amd.gmotion import (GM_AFFINE, GM_INLIER, GM_OUTLIER, global_motion_ref, model_flow, model_flow8,
                                projective_compensate_ref, projective_motion_ref, solve8, sums23)

_f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def pan_scene(w=256, h=128, f=300.0, deg=1.0):
    """the exact flow [h][w][2] (float64) of a pan by `deg` degrees about the vertical axis at a focal length of f px, and H"""
    t = np.deg2rad(deg)
    R = np.array([[np.cos(t), 0.0, np.sin(t)], [0.0, 1.0, 0.0], [-np.sin(t), 0.0, np.cos(t)]])
    K = np.diag([f, f, 1.0])
    Hm = K @ R @ np.linalg.inv(K)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    xs -= (w - 1) / 2.0
    ys -= (h - 1) / 2.0
    d = Hm[2, 0] * xs + Hm[2, 1] * ys + Hm[2, 2]
    return np.stack([(Hm[0, 0] * xs + Hm[0, 1] * ys + Hm[0, 2]) / d - xs, (Hm[1, 0] * xs + Hm[1, 1] * ys + Hm[1, 2]) / d - ys], -1), Hm


# ------------------------------------------------------------------ the sums
def test_the_sums_do_not_depend_on_the_order_of_the_pixels():
    rng = np.random.default_rng(5)
    for w, h in ((37, 11), (300, 70), (8192, 2)):
        flow = (rng.standard_normal((h, w, 2)) * 50).astype(_f32)
        sel = rng.random((h, w)) < 0.7
        want = sums23(flow, sel)
        assert want[:12] == gmotion.sums(flow, sel)   # the twelve sums of the affine fit come first
        for _ in range(3):
            assert sums23(flow, sel, rng.permutation(int(sel.sum()))) == want
        assert sums23(flow, sel, chunk=7) == want     # nor on how the pixels fall into workgroups


def test_the_sums_against_plain_python_integers():
    rng = np.random.default_rng(6)
    w, h = 9, 5
    flow = (rng.standard_normal((h, w, 2)) * 1000).astype(_f32)
    want = [0] * 23
    for y in range(h):
        for x in range(w):
            X, Y = 2 * x - (w - 1), 2 * y - (h - 1)
            qu, qv = (int(np.rint(flow[y, x, c] * _f32(256.0))) for c in (0, 1))
            terms = [1, X, Y, X * X, X * Y, Y * Y, qu, X * qu, Y * qu, qv, X * qv, Y * qv, X ** 3, X * X * Y, X * Y * Y, Y ** 3,
                     X ** 4, X ** 3 * Y, X * X * Y * Y, X * Y ** 3, Y ** 4, X * X * qu + X * Y * qv, X * Y * qu + Y * Y * qv]
            want = [a + b for a, b in zip(want, terms)]
    assert sums23(flow, np.ones((h, w), bool)) == want


def test_a_pair_needs_128_bits_and_a_workgroup_fits_64():
    """the sum of X^4 over 8192 x 2 pixels needs more than 63 bits; 1024 pixels (a workgroup's 256 quads) at the largest |X|, |Y|
    and |q| keep every sum of a record inside int64"""
    w, h = 8192, 2
    s = sums23(np.zeros((h, w, 2), _f32), np.ones((h, w), bool))
    assert s[16] == 2 * sum((2 * x - (w - 1)) ** 4 for x in range(w)) and s[16].bit_length() > 63
    assert gmotion.PM_BLOCK_PIXELS == 1024 and gmotion.PM_RECORD == 24 and gmotion.PM_NSUMS == 23
    X = Y = gmotion.GM_MAX_SIDE - 1
    q = int(gmotion.GM_MAX_FLOW * 256)
    worst = gmotion.PM_BLOCK_PIXELS * max(X ** 4, X * X * q + X * Y * q)
    assert worst < 1 << 63 and gmotion.PM_BLOCK_PIXELS * X ** 4 > 1 << 61
    with pytest.raises(AssertionError):
        sums23(np.zeros((h, w, 2), _f32), np.ones((h, w), bool), chunk=2048)


def test_wide_sums_convert_correctly_rounded():
    """float(int) is the conversion the header asks for: to nearest, ties to even, also past 64 bits and for negative sums"""
    for v, want in ((2 ** 70 + 2 ** 17, 2.0 ** 70), (2 ** 70 + 2 ** 17 + 1, 2.0 ** 70 + 2.0 ** 18), (2 ** 70 + 3 * 2 ** 17, 2.0 ** 70 + 2.0 ** 19),
                    (-(2 ** 64) - 1, -(2.0 ** 64)), (-5, -5.0), (2 ** 53 + 1, 2.0 ** 53)):
        assert float(v) == want


# ------------------------------------------------------------------ the solve
def test_a_noiseless_8_parameter_field_is_recovered():
    rng = np.random.default_rng(7)
    for w, h in ((64, 48), (301, 71), (6, 5)):
        a = rng.normal(0.0, 1.0, 8) * np.array([3.0, 0.02, 0.02, 3.0, 0.02, 0.02, 2e-4, 2e-4])
        flow = model_flow8(a, w, h).astype(_f32)[None]
        models, stats = projective_motion_ref(flow, rounds=1)
        assert stats[0].tolist() == [w * h, w * h, 8]
        # (the flow is rounded to float32 and quantised to 1/256 px: the parameters come back to that precision)
        assert np.abs(model_flow8(models[0], w, h) - model_flow8(a, w, h)).max() < 4e-3
        res, label = projective_compensate_ref(flow, models, thresh=0.01)
        assert (label == GM_INLIER).all() and np.abs(res).max() < 4e-3
    # a6 = a7 = 0: the affine field, with the quadratic terms found to be (nearly) zero
    a = np.array([1.5, 0.01, -0.02, -2.5, 0.015, 0.005, 0.0, 0.0])
    models, stats = projective_motion_ref(model_flow8(a, 64, 48).astype(_f32)[None], rounds=1)
    assert stats[0, 2] == 8 and np.abs(models[0, 6:]).max() < 1e-6 and np.allclose(models[0, :6], a[:6], atol=2e-3)


def _mask_of(sel):
    return np.where(sel, 0, 1).astype(np.uint8)[None]


def test_rank_deficient_sets_fall_back_to_global_motions_bits():
    rng = np.random.default_rng(8)
    H, W = 70, 300
    flow = (rng.standard_normal((1, H, W, 2)) * 2).astype(_f32)
    sets = {}
    sel = np.zeros((H, W), bool); sel[40, :] = True; sets["one row"] = (sel, 2)
    sel = np.zeros((H, W), bool); sel[np.arange(H), np.arange(H) + 17] = True; sets["one diagonal"] = (sel, 2)
    sel = np.zeros((H, W), bool); sel[:, 123] = True; sets["one column"] = (sel, 2)
    sel = np.zeros((H, W), bool); sel[7, 200] = True; sets["one pixel"] = (sel, 2)
    sel = np.zeros((H, W), bool); sel[[3, 50, 60], [10, 100, 290]] = True; sets["three pixels"] = (sel, 6)
    sel = np.zeros((H, W), bool); sets["nothing"] = (sel, 0)
    for name, (sel, count) in sets.items():
        models, stats = projective_motion_ref(flow, _mask_of(sel), rounds=1)
        m6, s6 = global_motion_ref(flow, _mask_of(sel), model=GM_AFFINE, rounds=1)
        assert stats[0].tolist() == [int(sel.sum()), int(sel.sum()), count], name
        assert np.array_equal(_bits(models[0, :6]), _bits(m6[0])) and not models[0, 6:].any(), name
        assert {6: 0, 2: 1, 0: 2}[count] == s6[0, 2], name
        if sel.sum() >= 4:   # what the rank test saw: a pivot that is zero, or rounding noise far below 2^-40
            assert abs(gmotion.pivot_ratios(sums23(flow[0], sel))[-1]) <= 2.3e-16, name
    # frames of one row or one column
    for shape in ((1, 1, 13, 2), (1, 9, 1, 2), (1, 1, 1, 2)):
        f = (rng.standard_normal(shape) * 2).astype(_f32)
        models, stats = projective_motion_ref(f, rounds=2)
        m6, s6 = global_motion_ref(f, rounds=2)
        assert stats[0, 2] == 2 and np.array_equal(_bits(models[0, :6]), _bits(m6[0])) and not models[0, 6:].any()


def test_small_legitimate_sets_pass_the_rank_test():
    rng = np.random.default_rng(9)
    # the 2 x 2 frame: 4 pixels, 8 equations, 8 unknowns
    f = (rng.standard_normal((1, 2, 2, 2)) * 2).astype(_f32)
    models, stats = projective_motion_ref(f, rounds=1)
    assert stats[0].tolist() == [4, 4, 8]
    assert np.abs(model_flow8(models[0], 2, 2) - f[0]).max() < 4e-3   # it interpolates its four pixels
    # a 2 x 2 block in the corner of a 300 x 70 frame: the smallest pivot ratio of a legitimate set, far above 2^-40
    H, W = 70, 300
    flow = (rng.standard_normal((1, H, W, 2)) * 2).astype(_f32)
    sel = np.zeros((H, W), bool)
    sel[:2, :2] = True
    ratio = min(gmotion.pivot_ratios(sums23(flow[0], sel)))
    assert 1e-11 < ratio < 1e-9 and ratio > 100 * gmotion.PM_PIVOT
    assert projective_motion_ref(flow, _mask_of(sel), rounds=1)[1][0, 2] == 8
    assert min(gmotion.pivot_ratios(sums23(flow[0], np.ones((H, W), bool)))) > 0.4


def test_rounds_and_an_emptying_set():
    two = np.zeros((2, 16, 24, 2), _f32)
    two[:, :, :12, 0], two[:, :, 12:, 0] = -20.0, 20.0
    two[1, :, :, 0] = 1.5
    want = projective_motion_ref(two, None, rounds=4, thresh=1e-3)
    first = projective_motion_ref(two, None, rounds=1, thresh=1e-3)
    assert np.array_equal(_bits(want[0][0]), _bits(first[0][0])) and want[1][0].tolist() == [384, 384, 8]
    assert (projective_compensate_ref(two, first[0], None, thresh=1e-3)[1][0] == GM_OUTLIER).all()
    shuffled = projective_motion_ref(two, None, rounds=4, thresh=1e-3, shuffle=np.random.default_rng(1))
    assert np.array_equal(_bits(shuffled[0]), _bits(want[0])) and np.array_equal(shuffled[1], want[1])
    with pytest.raises(ValueError):
        projective_motion_ref(two, rounds=9)
    with pytest.raises(ValueError):
        projective_compensate_ref(two, want[0], thresh=0.0)


def test_zero_quadratic_terms_give_the_affine_residual():
    rng = np.random.default_rng(10)
    flow = (rng.standard_normal((2, 11, 37, 2)) * 3).astype(_f32)
    flow[0, 3, 4] = np.nan
    m6, _ = global_motion_ref(flow, rounds=2)
    six = gmotion.motion_compensate_ref(flow, m6)
    eight = projective_compensate_ref(flow, np.concatenate([m6, np.zeros((2, 2))], 1))
    assert np.array_equal(six[0], eight[0], equal_nan=True) and np.array_equal(six[1], eight[1])


# ------------------------------------------------------------------ what the model is for
def test_a_one_degree_pan():
    """the exact flow of a 1 degree pan at f = 300 px on 256 x 128: the 8-parameter model's maximal error is below 0.01 px
    (0.0027), the affine fit's above 0.5 px (0.63), and a6 is -h31 / h33 within 1 % (0.04 %)"""
    w, h = 256, 128
    truth, Hm = pan_scene(w, h)
    flow = truth.astype(_f32)[None]
    m8, s8 = projective_motion_ref(flow, rounds=1)
    m6, _ = global_motion_ref(flow, rounds=1)
    err8 = np.abs(model_flow8(m8[0], w, h) - truth).max()
    err6 = np.abs(model_flow(m6[0], w, h) - truth).max()
    assert s8[0, 2] == 8
    assert err8 < 0.01
    assert err6 > 0.5
    assert abs(m8[0, 6] / (-Hm[2, 0] / Hm[2, 2]) - 1.0) < 0.01
    # the matrix form: to first order the model is the homography
    G = gmotion.homography(m8[0])
    assert G.shape == (3, 3) and np.abs(G / G[2, 2] - Hm / Hm[2, 2]).max() < 0.01
    assert np.array_equal(gmotion.homography(m6[0])[2], [0.0, 0.0, 1.0])


# ------------------------------------------------------------------ track selection
def test_track_select_ref_takes_8_wide_models():
    lmax, n = 6, 3
    size = (640, 480)
    a = np.array([4.0, 0.01, -0.006, -3.0, 0.004, 0.008, 3e-5, -2e-5])
    models = np.tile(a, (lmax, 1))
    pos = np.empty((lmax + 1, n, 2), _f32)
    pos[0] = np.array([[60, 50], [300, 200], [500, 90]], _f32)
    cx, cy = _f32(size[0] - 1) * _f32(0.5), _f32(size[1] - 1) * _f32(0.5)
    af = a.astype(_f32)
    for j in range(lmax):
        xc, yc = pos[j, :, 0] - cx, pos[j, :, 1] - cy
        pq = af[6] * xc + af[7] * yc
        pos[j + 1, :, 0] = pos[j, :, 0] + (((af[0] + af[1] * xc) + af[2] * yc) + pq * xc)
        pos[j + 1, :, 1] = pos[j, :, 1] + (((af[3] + af[4] * xc) + af[5] * yc) + pq * yc)
    start, length = np.zeros(n, np.int32), np.full(n, lmax + 1, np.int32)
    assert (tracking.track_select_ref(pos, start, length, models, size)[0] == tracking.TS_CAMERA).all()
    assert not tracking.track_select_ref(pos, start, length)[0].any()
    padded = tracking.track_select_ref(pos, start, length, np.concatenate([models[:, :6], np.zeros((lmax, 2))], 1), size)
    six = tracking.track_select_ref(pos, start, length, models[:, :6], size)
    assert all(np.array_equal(p, s, equal_nan=True) for p, s in zip(padded, six))
