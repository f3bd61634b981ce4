"""CPU: the numpy restatement of the global motion models and the motion-compensated flow (of_dis_amd/gmotion.py; the definition
is in include/ofdis.h above ofdis_global_motion) tested on its own: it recovers a known camera model from a scene with an
independently moving block, the trimming is what makes it do so, the sums do not depend on the order of their terms, and the
degenerate sets take the paths the header names.  The kernels are compared with it bit for bit in tests/test_gpu_gmotion.py."""
import numpy as np
import pytest

from of_dis_amd import gmotion
from of_dis_amd.gmotion import (GM_AFFINE, GM_EMPTY, GM_INLIER, GM_INVALID, GM_OK_AFFINE, GM_OUTLIER, GM_TRANSLATION,
                                GM_TRANSLATION_ONLY, global_motion_ref, motion_compensate_ref)

_f32 = np.float32
H, W = 112, 256
TRUE = np.array([2.5, 0.01, -0.004, -1.25, 0.006, 0.012])
BLOCK = (slice(30, 80), slice(60, 140))
HALF_DIAG = 0.5 * np.hypot(W - 1, H - 1)


def block_scene():
    """The camera model TRUE plus N(0, 0.1) noise, and a block that moves by (-6, 4) on its own: (flow [1][H][W][2], the
    noise-free camera flow [H][W][2])."""
    rng = np.random.default_rng(0)
    clean = gmotion.model_flow(TRUE, W, H)
    flow = (clean + rng.normal(0.0, 0.1, clean.shape)).astype(_f32)
    flow[BLOCK] = (-6.0, 4.0)
    return flow[None], clean


def errors(a):
    """(max translation error, max linear error x half-diagonal) in pixels"""
    d = np.abs(np.asarray(a) - TRUE)
    return max(d[0], d[3]), max(d[1], d[2], d[4], d[5]) * HALF_DIAG


def test_trimmed_rounds_recover_the_camera_model():
    flow, _ = block_scene()
    m1, s1 = global_motion_ref(flow, rounds=1, thresh=1.0)
    m3, s3 = global_motion_ref(flow, rounds=3, thresh=1.0)
    m5, s5 = global_motion_ref(flow, rounds=5, thresh=1.0)
    print("rounds 1:", s1[0], errors(m1[0]), " rounds 3:", s3[0], errors(m3[0]), " rounds 5:", s5[0], errors(m5[0]))
    assert s1[0].tolist() == [H * W, H * W, GM_OK_AFFINE]
    assert s3[0, 0] == H * W and s3[0, 2] == GM_OK_AFFINE
    assert s3[0, 1] == H * W - 50 * 80   # the last set is everything but the block
    assert max(errors(m3[0])) < 0.01
    assert errors(m1[0])[0] > 0.5        # the plain least-squares fit is pulled by the block
    assert np.array_equal(m5.view(np.uint64), m3.view(np.uint64)) and np.array_equal(s5, s3)


@pytest.mark.parametrize("model", [GM_TRANSLATION_ONLY, GM_AFFINE])
def test_the_order_of_the_terms_does_not_matter(model):
    flow, _ = block_scene()
    rng = np.random.default_rng(5)
    mask = rng.integers(0, 3, (1, H, W), dtype=np.uint8)
    for mk in (None, mask):
        want = global_motion_ref(flow, mk, model=model, rounds=3, thresh=1.0)
        for seed in (1, 2):
            got = global_motion_ref(flow, mk, model=model, rounds=3, thresh=1.0, shuffle=np.random.default_rng(seed))
            assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64))
            assert np.array_equal(got[1], want[1])


def test_translation_model_is_the_mean():
    flow, _ = block_scene()
    m, s = global_motion_ref(flow, model=GM_TRANSLATION_ONLY, rounds=1)
    assert s[0, 2] == GM_TRANSLATION and not m[0, [1, 2, 4, 5]].any()
    q = np.rint(flow[0].astype(np.float64) * 256.0)
    assert abs(m[0, 0] - q[..., 0].mean() / 256.0) < 1e-12 and abs(m[0, 3] - q[..., 1].mean() / 256.0) < 1e-12


def _keep_only(sel):
    """a mask [1][H][W] that is OFDIS_FB_CONSISTENT on `sel` only"""
    mask = np.full((1, H, W), 1, np.uint8)
    mask[0][sel] = 0
    return mask


@pytest.mark.parametrize("which", ["row", "diagonal"])
def test_collinear_sets_fall_back_to_the_translation(which):
    """one row or one diagonal of the 256x112 frame: every product of the solve is exact, det == 0.0"""
    flow, _ = block_scene()
    sel = np.zeros((H, W), bool)
    if which == "row":
        sel[40, :] = True
    else:
        sel[np.arange(H), np.arange(H) + 17] = True
    s = gmotion.sums(flow[0], sel)
    n, Sx, Sy, Sxx, Sxy, Syy = (float(v) for v in s[:6])
    det = (n * (Sxx * Syy - Sxy * Sxy) + Sx * (Sxy * Sy - Sx * Syy)) + Sy * (Sx * Sxy - Sxx * Sy)
    assert det == 0.0 and s[0] >= 3
    m, st = global_motion_ref(flow, _keep_only(sel), rounds=1)
    assert st[0].tolist() == [int(sel.sum()), int(sel.sum()), GM_TRANSLATION]
    assert not m[0, [1, 2, 4, 5]].any()
    assert abs(m[0, 0] - flow[0][sel][:, 0].astype(np.float64).mean()) < 1.0 / 256


def test_a_single_valid_pixel_gives_its_own_flow():
    flow, _ = block_scene()
    sel = np.zeros((H, W), bool)
    sel[7, 200] = True
    m, st = global_motion_ref(flow, _keep_only(sel), rounds=3, thresh=1.0)
    assert st[0].tolist() == [1, 1, GM_TRANSLATION]
    q = np.rint(flow[0, 7, 200].astype(np.float64) * 256.0) / 256.0
    assert m[0].tolist() == [q[0], 0.0, 0.0, q[1], 0.0, 0.0]


def test_an_all_masked_frame_is_empty():
    flow, _ = block_scene()
    for mask in (np.full((1, H, W), 1, np.uint8), np.full((1, H, W), 2, np.uint8)):
        m, st = global_motion_ref(flow, mask, rounds=3)
        assert st[0].tolist() == [0, 0, GM_EMPTY] and not m.any()
    bad = np.full((1, 4, 6, 2), np.nan, _f32)
    bad[0, 0, 0] = (np.inf, 0.0)
    bad[0, 1, 1] = (0.0, 4096.5)
    m, st = global_motion_ref(bad, rounds=2)
    assert st[0].tolist() == [0, 0, GM_EMPTY] and not m.any()
    res, label = motion_compensate_ref(bad, m)
    assert (label == GM_INVALID).all() and np.isnan(res[0, 2, 2]).all() and res[0, 0, 0, 0] == np.inf


def test_a_set_that_empties_keeps_the_previous_round():
    """two halves that move apart by 40 px: the least-squares model of round 0 is more than 1e-3 px from every pixel (checked
    here), so round 1's set is empty at thresh 1e-3 and round 0's model, set size and status stay"""
    flow = np.zeros((1, 16, 24, 2), _f32)
    flow[0, :, :12, 0] = -20.0
    flow[0, :, 12:, 0] = 20.0
    m1, s1 = global_motion_ref(flow, rounds=1, thresh=1e-3)
    res, label = motion_compensate_ref(flow, m1, thresh=1e-3)
    assert (label == GM_OUTLIER).all()                      # the set round 1 would use is empty
    for rounds in (2, 4):
        m, s = global_motion_ref(flow, rounds=rounds, thresh=1e-3)
        assert np.array_equal(m.view(np.uint64), m1.view(np.uint64)) and np.array_equal(s, s1)
    assert s1[0].tolist() == [16 * 24, 16 * 24, GM_OK_AFFINE]


@pytest.mark.parametrize("rounds", [1, 2, 3])
def test_inlier_labels_are_the_next_rounds_set(rounds):
    """label == INLIER under the model of `rounds` rounds is the set round `rounds` sums over: its size is what one more round
    reports as the last set used"""
    flow, _ = block_scene()
    rng = np.random.default_rng(11)
    mask = (rng.random((1, H, W)) < 0.1).astype(np.uint8) * rng.integers(1, 3, (1, H, W), dtype=np.uint8)
    m, _ = global_motion_ref(flow, mask, rounds=rounds, thresh=1.0)
    res, label = motion_compensate_ref(flow, m, mask, thresh=1.0)
    m_next, s_next = global_motion_ref(flow, mask, rounds=rounds + 1, thresh=1.0)
    assert int((label == GM_INLIER).sum()) == s_next[0, 1] > 0
    sel = label[0] == GM_INLIER
    a, status = gmotion.solve(gmotion.sums(flow[0], sel), GM_AFFINE)
    assert np.array_equal(a.view(np.uint64), m_next[0].view(np.uint64)) and status == s_next[0, 2]
    assert ((label == GM_INVALID) == (mask != 0)).all()
    assert (label[0][BLOCK][mask[0][BLOCK] == 0] == GM_OUTLIER).all()


def test_the_residual_of_a_noise_free_affine_flow_vanishes():
    clean = gmotion.model_flow(TRUE, W, H).astype(_f32)[None]
    m, s = global_motion_ref(clean, rounds=2, thresh=1.0)
    res, label = motion_compensate_ref(clean, m, thresh=1.0)
    print("max |residual|", np.abs(res).max(), "model error", np.abs(m[0] - TRUE).max())
    assert np.abs(res).max() < 1e-3 and (label == GM_INLIER).all()
    assert s[0].tolist() == [H * W, H * W, GM_OK_AFFINE]


def test_argument_errors():
    flow, _ = block_scene()
    for kw in (dict(rounds=0), dict(rounds=9), dict(thresh=0.0), dict(thresh=-1.0), dict(thresh=np.nan), dict(thresh=np.inf),
               dict(model=2)):
        with pytest.raises(ValueError):
            global_motion_ref(flow, **kw)
