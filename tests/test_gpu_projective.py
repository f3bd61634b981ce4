"""-m gpu: the 8-parameter projective camera models (include/ofdis.h, "Projective camera models": ofdis_projective_motion /
ofdis_projective_compensate on materialised arrays, ofdis_batch_projective_motion / ofdis_batch_projective_compensate straight
from the level flows of a context, ofdis_track_select_projective).

As tests/test_gpu_gmotion.py does for the 6-parameter calls, with the cases and the checks both orders take from
tests/camera_cases.py: the standalone kernels are compared bit for bit -- models as raw 64-bit patterns, stats, residual (NaN
payloads included) and label -- with of_dis_amd/gmotion.py, the header's definition in numpy; the fused kernels bit for bit with
the standalone ones applied to the outputs of ofdis_batch_upsample_bidir (fb_check = 1) or ofdis_batch_upsample_frames (fb_check
= 0).  Conditions on the generated inputs are checked on the restatement or the standalone result, never on the kernel under
test."""
import numpy as np
import pytest

import camera_cases as cases
import gen_synth
from camera_cases import _keep_only, _random_case, assert_compensated_equal, assert_fit_equal
from of_dis_amd import gmotion, tracking
from of_dis_amd.gmotion import (GM_INLIER, GM_INVALID, GM_OUTLIER, global_motion_ref, motion_compensate_ref,
                                projective_compensate_ref, projective_motion_ref)
from of_dis_amd.tracking import TrackSelectParams, track_select_ref
from seq_products import assert_same_bits, run_context, smooth_clip

pytestmark = pytest.mark.gpu
_f32 = np.float32


# ------------------------------------------------------------------ 1. standalone kernels against the restatement
# 1x1, 13x1, 1x9: the fallbacks; 2x2: the smallest full-rank set; 300x70: several records per pair; 8192x2: the pair's sums need
# 128 bits and a workgroup's come near the int64 bound
SIZES = [(1, 1), (13, 1), (1, 9), (2, 2), (6, 5), (37, 11), (64, 16), (257, 3), (300, 70), (8192, 2)]
# (rounds, thresh): rounds 1, 2, 4 and thresh 1.0, 0.5, 1e-3
FITS = [(1, 1.0), (2, 0.5), (4, 1.0), (4, 1e-3), (2, 1e-3), (1, 0.5)]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("kind", ["smooth", "wild"])
def test_standalone_matches_the_definition(gpu, w, h, kind):
    counts = set()
    for npairs in (1, 3):
        flow, mask = _random_case(npairs, w, h, kind)
        for mk in (mask, None):
            for rounds, thresh in FITS:
                what = f"{w}x{h}, {kind}, {npairs} pairs, mask {mk is not None}, rounds {rounds}, thresh {thresh}"
                want = projective_motion_ref(flow, mk, rounds=rounds, thresh=thresh)
                assert_fit_equal(gpu.projective_motion(flow, mk, rounds=rounds, thresh=thresh), want, what)
                counts |= set(want[1][:, 2].tolist())
                if rounds in (1, 4):   # the pass with the models just compared
                    wantc = projective_compensate_ref(flow, want[0], mk, thresh=thresh)
                    assert_compensated_equal(gpu.projective_compensate(flow, want[0], mk, thresh=thresh), wantc, what)
    # which branch the size exercises (condition on the restatement)
    if w == 1 or h == 1:
        assert 8 not in counts and 6 not in counts
    elif w * h >= 30:
        assert 8 in counts
    if (w, h) == (2, 2) and kind == "smooth":
        assert projective_motion_ref(_random_case(1, 2, 2, "smooth")[0], None, rounds=1)[1][0].tolist() == [4, 4, 8]


def test_the_pair_sums_need_128_bits_and_the_largest_right_hand_sides(gpu):
    """8192 x 2 with |u| = |v| = 4096 everywhere: the largest R6 / R7 terms, and fourth moments past 63 bits"""
    w, h = 8192, 2
    flow = np.empty((2, h, w, 2), _f32)
    flow[0, ..., 0], flow[0, ..., 1] = 4096.0, -4096.0
    flow[1, :, : w // 2, 0], flow[1, :, w // 2:, 0] = -4096.0, 4096.0
    flow[1, ..., 1] = np.where(np.arange(w) % 2 == 0, 4096.0, -4096.0)[None, :]
    s = gmotion.sums23(flow[0], np.ones((h, w), bool))
    assert s[16].bit_length() > 63 and abs(s[21]).bit_length() > 57   # (int64 would overflow; R6 at its per-pixel maximum)
    for rounds in (1, 2):
        want = projective_motion_ref(flow, None, rounds=rounds, thresh=1.0)
        assert_fit_equal(gpu.projective_motion(flow, None, rounds=rounds, thresh=1.0), want, f"rounds {rounds}")
    assert_compensated_equal(gpu.projective_compensate(flow, want[0], None, thresh=1.0),
                             projective_compensate_ref(flow, want[0], None, thresh=1.0), "largest products")


def test_degenerate_sets(gpu):
    """the degenerate sets of tests/test_gpu_gmotion.py::test_degenerate_sets as five pairs of ONE call: a row, a diagonal, a single
    pixel, nothing, everything -- the counts are the restatement's"""
    import test_gmotion_ref as R
    H, W = R.H, R.W
    flow = np.repeat(R.block_scene()[0], 5, axis=0)
    sel = np.zeros((5, H, W), bool)
    sel[0, 40, :] = True
    sel[1, np.arange(H), np.arange(H) + 17] = True
    sel[2, 7, 200] = True
    sel[4] = True
    mask = _keep_only((5, H, W), sel)
    mask[3] = np.random.default_rng(3).integers(1, 3, (H, W), dtype=np.uint8)
    want = projective_motion_ref(flow, mask, rounds=3, thresh=1.0)
    affine = global_motion_ref(flow, mask, rounds=3, thresh=1.0)
    assert want[1][:, 2].tolist() == [2, 2, 2, 0, 8] and want[1][:, 0].tolist() == [W, H, 1, 0, H * W]
    assert_same_bits(want[0][:4, :6], affine[0][:4], "the fallbacks are ofdis_global_motion's bits")
    assert not want[0][:4, 6:].any()
    assert_fit_equal(gpu.projective_motion(flow, mask, rounds=3, thresh=1.0), want, "degenerate sets")
    wantc = projective_compensate_ref(flow, want[0], mask, thresh=1.0)
    assert (wantc[1][3] == GM_INVALID).all()
    assert_compensated_equal(gpu.projective_compensate(flow, want[0], mask, thresh=1.0), wantc, "degenerate sets")
    # a set that empties at round 1 keeps round 0's model, set size and count (next to a pair that goes on)
    two = np.zeros((2, 16, 24, 2), _f32)
    two[:, :, :12, 0], two[:, :, 12:, 0] = -20.0, 20.0
    two[1, :, :, 0] = 1.5
    want = projective_motion_ref(two, None, rounds=4, thresh=1e-3)
    first = projective_motion_ref(two, None, rounds=1, thresh=1e-3)
    assert np.array_equal(want[0][0], first[0][0]) and want[1][0].tolist() == [384, 384, 8]
    assert_fit_equal(gpu.projective_motion(two, None, rounds=4, thresh=1e-3), want, "a set that empties")


def test_more_pairs_than_xcds(gpu):
    cases.check_more_pairs_than_xcds(gpu, 8)


@pytest.mark.parametrize("w,h", [(64, 16), (37, 11), (6, 5)], ids=["64x16", "37x11", "6x5"])
def test_unaligned_outputs_take_narrower_stores_with_the_same_bytes(gpu, w, h):
    cases.check_unaligned_outputs(gpu, 8, w, h)


def test_either_output_alone_the_residual_in_place_and_no_stats(gpu):
    cases.check_either_output_alone_in_place_and_no_stats(gpu, 8)


# ------------------------------------------------------------------ 2. cross-checks with the 6-parameter calls
def test_models_padded_with_zeros_give_the_6_parameter_outputs(gpu):
    for w, h in ((37, 11), (64, 16), (300, 70)):
        flow, mask = _random_case(3, w, h, "wild")
        m6, _ = global_motion_ref(flow, mask, rounds=2, thresh=1.0)
        m8 = np.concatenate([m6, np.zeros((3, 2))], axis=1)
        six = gpu.motion_compensate(flow, m6, mask, thresh=1.0)
        eight = gpu.projective_compensate(flow, m8, mask, thresh=1.0)
        assert np.array_equal(six[0], eight[0], equal_nan=True) and np.array_equal(six[1], eight[1]), (w, h)


# ------------------------------------------------------------------ 3. track selection under 8-parameter models
def _models8(af, seed):
    """the affine models of the population with quadratic terms of a few 1e-5 per pixel^2 (a pixel at the frame's edge)"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.concatenate([af, rng.uniform(-4e-5, 4e-5, (len(af), 2))], axis=1))


TS_CASES = [(n, lmax) for lmax in (1, 2, 15) for n in (1, 17, 200)]


@pytest.mark.parametrize("n,lmax", TS_CASES, ids=[f"n{n}-L{lmax}" for n, lmax in TS_CASES])
def test_track_select_under_projective_models(gpu, n, lmax):
    """the cases of tests/test_gpu_track_select.py with 8-wide models: the definition's bits; with two zeros appended to the
    affine models, the outputs of ofdis_track_select"""
    from test_track_select_ref import SIZE, population
    tracks, start, length, _, af = population(200, lmax)
    tracks, start, length = tracks[:, :n], start[:n], length[:n]
    m8 = _models8(af, lmax)
    want = track_select_ref(tracks, start, length, m8, SIZE)
    got = gpu.track_select(tracks, start, length, m8, SIZE)
    for g, w_, name in zip(got, want, ("code", "counts", "tracks", "start", "len", "info", "index", "shape")):
        assert_same_bits(np.ascontiguousarray(g), np.ascontiguousarray(w_), f"n {n} lmax {lmax}: {name}")
    padded = gpu.track_select(tracks, start, length, np.concatenate([af, np.zeros((len(af), 2))], axis=1), SIZE)
    six = gpu.track_select(tracks, start, length, af, SIZE)
    for g, w_ in zip(padded, six):
        assert np.array_equal(g, w_, equal_nan=True)


def test_a_track_that_follows_a_projective_model_is_camera(gpu):
    from test_track_select_ref import SIZE
    lmax, n = 8, 5
    a = np.array([4.0, 0.01, -0.006, -3.0, 0.004, 0.008, 3e-5, -2e-5])
    models = np.tile(a, (lmax, 1))
    pos = np.empty((lmax + 1, n, 2), _f32)
    pos[0] = np.array([[60, 50], [300, 200], [500, 90], [100, 300], [320, 240]], _f32)[:n]
    cx, cy = _f32(SIZE[0] - 1) * _f32(0.5), _f32(SIZE[1] - 1) * _f32(0.5)
    af = a.astype(_f32)
    for j in range(lmax):   # the header's fp32 expression: every step equals the model there up to the rounding of the sum
        xc, yc = pos[j, :, 0] - cx, pos[j, :, 1] - cy
        pq = af[6] * xc + af[7] * yc
        pos[j + 1, :, 0] = pos[j, :, 0] + (((af[0] + af[1] * xc) + af[2] * yc) + pq * xc)
        pos[j + 1, :, 1] = pos[j, :, 1] + (((af[3] + af[4] * xc) + af[5] * yc) + pq * yc)
    start, length = np.zeros(n, np.int32), np.full(n, lmax + 1, np.int32)
    want = track_select_ref(pos, start, length, models, SIZE)
    assert (want[0] == tracking.TS_CAMERA).all() and not track_select_ref(pos, start, length)[0].any()
    assert (track_select_ref(pos, start, length, models[:, :6], SIZE)[0] == 0).any()   # the affine part alone does not explain them
    got = gpu.track_select(pos, start, length, models, SIZE)
    assert_same_bits(got[0], want[0], "codes with the model")
    assert not gpu.track_select(pos, start, length)[0].any()


# ------------------------------------------------------------------ 4. fused kernels against the standalone ones
FUSED_FITS = [(3, 1.0), (2, 0.5)]
# (kind, noc, w, h, n pairs, first, count, pipeline, contract, alpha, beta)
FUSED_CASES = [
    pytest.param("seq_rev", 1, 256, 112, 3, 0, 3, 1, 0, 0.01, 0.5, id="gray"),
    pytest.param("seq_rev", 3, 256, 112, 3, 0, 3, 1, 0, 0.01, 0.5, id="rgb"),
    pytest.param("seq_rev", 1, 250, 110, 3, 0, 3, 1, 0, 0.01, 0.5, id="gray-crop-250x110"),
    pytest.param("reverse", 3, 243, 107, 2, 0, 2, 1, 0, 0.01, 0.5, id="rgb-crop-243x107-reverse"),
    pytest.param("plain", 1, 250, 110, 3, 0, 3, 1, 0, 0.01, 0.5, id="gray-crop-250x110-plain"),
    pytest.param("seq_rev", 1, 256, 112, 5, 1, 3, 1, 0, 0.01, 0.5, id="gray-subrange-1-3-of-5"),
    pytest.param("seq_rev", 1, 256, 112, 16, 0, 16, 2, 0, 0.01, 0.5, id="gray-16-pairs-pipelined"),
    pytest.param("seq_rev", 1, 256, 112, 3, 0, 3, 1, 1, 0.01, 0.5, id="gray-fused-contract"),
    pytest.param("reverse", 3, 256, 112, 2, 0, 2, 1, 1, 0.01, 0.5, id="rgb-fused-contract"),
    pytest.param("seq_rev", 1, 256, 112, 3, 0, 3, 1, 0, 0.0, 0.0, id="gray-alpha0-beta0"),
]


@pytest.mark.parametrize("kind,noc,w,h,n,first,count,pipeline,contract,alpha,beta", FUSED_CASES)
def test_fused_matches_standalone(gpu, kind, noc, w, h, n, first, count, pipeline, contract, alpha, beta):
    fits = [dict(rounds=rounds, thresh=thresh) for rounds, thresh in FUSED_FITS]
    cases.check_fused_matches_standalone(gpu, 8, fits, kind, noc, 2, w, h, n, first, count, pipeline, contract, alpha, beta)


# ------------------------------------------------------------------ 5. end to end
def pan_homography(deg, f):
    """H = K R K^-1 of a pan by `deg` degrees about the vertical axis at a focal length of f pixels, in centred coordinates"""
    t = np.deg2rad(deg)
    R = np.array([[np.cos(t), 0.0, np.sin(t)], [0.0, 1.0, 0.0], [-np.sin(t), 0.0, np.cos(t)]])
    K = np.diag([f, f, 1.0])
    return K @ R @ np.linalg.inv(K)


def homography_flow(Hm, w, h):
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    xs -= (w - 1) / 2.0
    ys -= (h - 1) / 2.0
    d = Hm[2, 0] * xs + Hm[2, 1] * ys + Hm[2, 2]
    return np.stack([(Hm[0, 0] * xs + Hm[0, 1] * ys + Hm[0, 2]) / d - xs, (Hm[1, 0] * xs + Hm[1, 1] * ys + Hm[1, 2]) / d - ys], -1)


def test_end_to_end_pan(gpu):
    """One 256x128 gray pair: A the central window of gen_synth._texture(default_rng(77), 128, 256), B the same texture sampled
    with cubic map_coordinates at H^-1 of a 1 degree pan about the vertical axis at f = 300 px.  Operating point 2, fb_check = 0,
    rounds 3, thresh 1: the mean distance between the model field and the true homography field for the 8-parameter and the
    affine fit.  On the CPU restatement these are 0.036 px and 0.289 px.
    Measured on an MI355X: 0.0356 px for the 8-parameter fit (32662 of 32768 pixels in the last set) and 0.2891 px for the affine
    fit, a ratio of 0.123; a6 = 5.24e-05 against -h31/h33 = 5.82e-05.  The bounds are the issue's: a quarter of the affine error,
    and 0.1 px."""
    from scipy.ndimage import map_coordinates
    w, h = 256, 128
    tex = gen_synth._texture(np.random.default_rng(77), 128, 256)
    th, tw = tex.shape
    y0, x0 = (th - h) // 2, (tw - w) // 2
    Hm = pan_homography(1.0, 300.0)
    truth = homography_flow(Hm, w, h)
    # B(x') = A(H^-1 x'): the content of A at x appears in B at H x, so the flow of A -> B is H x - x
    back = homography_flow(np.linalg.inv(Hm), w, h)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    B = map_coordinates(tex, [ys + back[..., 1] + y0, xs + back[..., 0] + x0], order=3, mode="nearest")
    to_u8 = lambda t: np.clip(np.rint(t), 0, 255).astype(np.uint8)
    A, B = to_u8(tex[y0:y0 + h, x0:x0 + w]), to_u8(B)
    b, devs = run_context(gpu, np.stack([A, B]), "plain")
    try:
        m8, s8 = b.projective_motion(w, h, rounds=3, thresh=1.0, fb_check=False)
        m6, s6 = b.global_motion(w, h, rounds=3, thresh=1.0, fb_check=False)
    finally:
        b.close()
    dist = lambda field: float(np.hypot(*np.moveaxis(field - truth, -1, 0)).mean())
    err8, err6 = dist(gmotion.model_flow8(m8[0], w, h)), dist(gmotion.model_flow(m6[0], w, h))
    print(f"pan 1 deg, f 300: mean error of the 8-parameter fit {err8:.4f} px, of the affine fit {err6:.4f} px, ratio "
          f"{err8 / err6:.3f}; stats {s8[0].tolist()} {s6[0].tolist()}; a6 {m8[0, 6]:.4e} against {-Hm[2, 0] / Hm[2, 2]:.4e}")
    assert s8[0, 2] == 8
    assert err8 < err6 / 4
    assert err8 < 0.1


# ------------------------------------------------------------------ 6. the command-line tool
def test_camera_motion_tool_projective(gpu, tmp_path):
    """tools/camera_motion.py --model projective on three PNGs: the CSV holds Batch.projective_motion's bits"""
    import os
    import subprocess
    import sys
    from PIL import Image
    w, h, n = 250, 107, 2
    clip = smooth_clip(w, h, 1, n + 1)
    paths = []
    for k, f in enumerate(clip):
        paths.append(str(tmp_path / f"f{k}.png"))
        Image.fromarray(f).save(paths[-1])
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "camera_motion.py")
    csv, stem = str(tmp_path / "cam.csv"), str(tmp_path / "lab")
    res = subprocess.run([sys.executable, tool, "--model", "projective", "--rounds", "2", "--thresh", "0.75", "--labels", stem]
                         + paths + [csv], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout, res.stderr)
    b, devs = run_context(gpu, clip)
    try:
        models, stats = b.projective_motion(w, h, rounds=2, thresh=0.75, fb_check=True)
        label = b.projective_compensate(models, w, h, thresh=0.75, fb_check=True, residual=False)[1]
    finally:
        b.close()
    rows = [line.split(",") for line in open(csv).read().splitlines()]
    assert len(rows) == n and all(len(r) == 11 for r in rows)
    assert_same_bits(np.array([[float(v) for v in r[:8]] for r in rows], np.float64), models, "the tool's models")
    assert_same_bits(np.array([[int(v) for v in r[8:]] for r in rows], np.int64), stats, "the tool's stats")
    assert (stats[:, 2] == 8).all()
    grey = np.array([0, 127, 255], np.uint8)
    for k in range(n):
        assert_same_bits(np.asarray(Image.open(f"{stem}_{k:03d}.png")), grey[label[k]], f"label map {k}")
