"""-m gpu: global motion models and motion-compensated flow (include/ofdis.h: ofdis_global_motion / ofdis_motion_compensate on
materialised arrays, ofdis_batch_global_motion / ofdis_batch_motion_compensate straight from the level flows of a context).

The standalone kernels are compared bit for bit -- models as raw 64-bit patterns, stats, residual (NaN payloads included) and
label -- with of_dis_amd/gmotion.py, the header's definition in numpy; the fused kernels bit for bit with the standalone ones
applied to the outputs of ofdis_batch_upsample_bidir (fb_check = 1) or ofdis_batch_upsample_frames (fb_check = 0).  Conditions
on the generated inputs are checked on the restatement or the standalone result, never on the kernel under test."""
import math

import numpy as np
import pytest

import camera_cases as cases
import gen_synth
from camera_cases import _keep_only, _random_case, assert_compensated_equal, assert_fit_equal
from of_dis_amd import gmotion
from of_dis_amd.gmotion import (GM_AFFINE, GM_EMPTY, GM_INLIER, GM_INVALID, GM_OK_AFFINE, GM_OUTLIER, GM_TRANSLATION,
                                GM_TRANSLATION_ONLY, global_motion_ref, motion_compensate_ref)
from seq_products import (FB_REJECTS, INVALID, RANGE_REJECTS, SIZE_REJECTS, assert_same_bits, flag_contexts, run_context,
                          smooth_clip)

pytestmark = pytest.mark.gpu
_f32 = np.float32


# ------------------------------------------------------------------ 1. standalone kernels against the restatement
# (300, 70): several workgroups per pair, so the slab sum is real; (8192, 2): |X| at its bound
SIZES = [(37, 11), (64, 16), (1, 9), (13, 1), (1, 1), (6, 5), (33, 7), (257, 3), (300, 70), (8192, 2)]
# (model, rounds, thresh)
FITS = [(GM_AFFINE, 1, 1.0), (GM_AFFINE, 2, 0.5), (GM_AFFINE, 4, 1.0), (GM_AFFINE, 4, 1e-3), (GM_TRANSLATION_ONLY, 1, 0.5),
        (GM_TRANSLATION_ONLY, 2, 1.0), (GM_TRANSLATION_ONLY, 4, 0.5), (GM_TRANSLATION_ONLY, 2, 1e-3)]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("kind", ["smooth", "wild"])
def test_standalone_matches_the_definition(gpu, w, h, kind):
    gated_away = 0
    for npairs in (1, 3):
        flow, mask = _random_case(npairs, w, h, kind)
        for mk in (mask, None):
            for model, rounds, thresh in FITS:
                what = f"{w}x{h}, {kind}, {npairs} pairs, mask {mk is not None}, model {model}, rounds {rounds}, thresh {thresh}"
                want = global_motion_ref(flow, mk, model=model, rounds=rounds, thresh=thresh)
                assert_fit_equal(gpu.global_motion(flow, mk, model=model, rounds=rounds, thresh=thresh), want, what)
                if rounds > 1:
                    gated_away += int((want[1][:, 1] < want[1][:, 0]).sum())
                if rounds in (1, 4):   # the pass with the models just compared
                    wantc = motion_compensate_ref(flow, want[0], mk, thresh=thresh)
                    assert_compensated_equal(gpu.motion_compensate(flow, want[0], mk, thresh=thresh), wantc, what)
    if kind == "smooth" and w * h >= 9:   # the gate really removes pixels in this case (condition on the restatement)
        assert gated_away > 0


def test_either_output_alone_and_the_residual_in_place(gpu):
    cases.check_either_output_alone_in_place_and_no_stats(gpu, 6)


def test_more_pairs_than_xcds(gpu):
    cases.check_more_pairs_than_xcds(gpu, 6)


def test_the_largest_products(gpu):
    """8192 x 2 with |u| = 4096 everywhere: X * qu reaches 8191 * 2^20, past 32 bits, in every lane"""
    w, h = 8192, 2
    flow = np.empty((2, h, w, 2), _f32)
    flow[0, ..., 0], flow[0, ..., 1] = 4096.0, -4096.0
    flow[1, :, : w // 2, 0], flow[1, :, w // 2:, 0] = -4096.0, 4096.0    # SXqu = sum |X| * 2^20
    flow[1, ..., 1] = np.where(np.arange(w) % 2 == 0, 4096.0, -4096.0)[None, :]
    for model in (GM_AFFINE, GM_TRANSLATION_ONLY):
        want = global_motion_ref(flow, None, model=model, rounds=2, thresh=1.0)
        assert_fit_equal(gpu.global_motion(flow, None, model=model, rounds=2, thresh=1.0), want, f"model {model}")
    s = gmotion.sums(flow[1], np.ones((h, w), bool))
    assert s[7] == 2 * sum(abs(2 * x - (w - 1)) for x in range(w)) << 20 > 1 << 45


def test_degenerate_sets(gpu):
    """the degenerate cases of tests/test_gmotion_ref.py on the kernels: collinear sets (det == 0.0 exactly: translation), a
    single pixel, an all-masked frame and a set that empties -- one pair each of ONE call, so that the pairs take different paths
    side by side"""
    import test_gmotion_ref as R
    H, W = R.H, R.W
    flow = np.repeat(R.block_scene()[0], 5, axis=0)
    sel = np.zeros((5, H, W), bool)
    sel[0, 40, :] = True
    sel[1, np.arange(H), np.arange(H) + 17] = True
    sel[2, 7, 200] = True
    sel[4] = True          # pair 3: nothing; pair 4: everything
    mask = _keep_only((5, H, W), sel)
    mask[3] = np.random.default_rng(3).integers(1, 3, (H, W), dtype=np.uint8)
    want = global_motion_ref(flow, mask, rounds=3, thresh=1.0)
    assert want[1][:, 2].tolist() == [GM_TRANSLATION, GM_TRANSLATION, GM_TRANSLATION, GM_EMPTY, GM_OK_AFFINE]
    assert want[1][:, 0].tolist() == [W, H, 1, 0, H * W]
    assert_fit_equal(gpu.global_motion(flow, mask, rounds=3, thresh=1.0), want, "degenerate sets")
    wantc = motion_compensate_ref(flow, want[0], mask, thresh=1.0)
    assert (wantc[1][3] == GM_INVALID).all()
    assert_compensated_equal(gpu.motion_compensate(flow, want[0], mask, thresh=1.0), wantc, "degenerate sets")
    # a set that empties at round 1 keeps round 0's model, set size and status (next to a pair that goes on)
    two = np.zeros((2, 16, 24, 2), _f32)
    two[:, :, :12, 0], two[:, :, 12:, 0] = -20.0, 20.0
    two[1, :, :, 0] = 1.5
    want = global_motion_ref(two, None, rounds=4, thresh=1e-3)
    first = global_motion_ref(two, None, rounds=1, thresh=1e-3)
    assert np.array_equal(want[0][0], first[0][0]) and want[1][0].tolist() == [384, 384, GM_OK_AFFINE]
    assert (motion_compensate_ref(two, first[0], None, thresh=1e-3)[1][0] == GM_OUTLIER).all()
    assert_fit_equal(gpu.global_motion(two, None, rounds=4, thresh=1e-3), want, "a set that empties")


@pytest.mark.parametrize("w,h", [(64, 16), (37, 11), (6, 5)], ids=["64x16", "37x11", "6x5"])
def test_unaligned_outputs_take_narrower_stores_with_the_same_bytes(gpu, w, h):
    cases.check_unaligned_outputs(gpu, 6, w, h)


# ------------------------------------------------------------------ 2. the block scene
def test_block_scene_on_the_kernel(gpu):
    """the scene of tests/test_gmotion_ref.py through the standalone kernel: the restatement's bits, which carry its < 0.01 px"""
    import test_gmotion_ref as R
    flow, _ = R.block_scene()
    for rounds in (1, 3, 5):
        want = global_motion_ref(flow, None, rounds=rounds, thresh=1.0)
        assert_fit_equal(gpu.global_motion(flow, None, rounds=rounds, thresh=1.0), want, f"block scene, rounds {rounds}")
        if rounds == 3:
            assert max(R.errors(want[0][0])) < 0.01
            wantc = motion_compensate_ref(flow, want[0], None, thresh=1.0)
            assert (wantc[1][0][R.BLOCK] == GM_OUTLIER).all() and (wantc[1] == GM_INLIER).sum() == want[1][0, 1]
            assert_compensated_equal(gpu.motion_compensate(flow, want[0], None, thresh=1.0), wantc, "block scene")


# ------------------------------------------------------------------ 3. fused kernels against the standalone ones
FUSED_FITS = [(GM_AFFINE, 3, 1.0), (GM_TRANSLATION_ONLY, 2, 0.5)]

# (kind, noc, op, w, h, n pairs, first, count, pipeline, contract, alpha, beta)
FUSED_CASES = [
    pytest.param("seq_rev", 1, 2, 256, 112, 3, 0, 3, 1, 0, 0.01, 0.5, id="gray-op2-scl1"),
    pytest.param("seq_rev", 3, 2, 256, 112, 3, 0, 3, 1, 0, 0.01, 0.5, id="rgb-op2-scl1"),
    pytest.param("seq_rev", 1, 4, 256, 112, 2, 0, 2, 1, 0, 0.01, 0.5, id="gray-op4-scl0"),
    pytest.param("reverse", 3, 4, 256, 112, 2, 0, 2, 1, 0, 0.01, 0.5, id="rgb-op4-scl0-reverse"),
    pytest.param("seq_rev", 1, 2, 250, 110, 3, 0, 3, 1, 0, 0.01, 0.5, id="gray-crop-250x110"),
    pytest.param("seq_rev", 3, 2, 243, 107, 2, 0, 2, 1, 0, 0.01, 0.5, id="rgb-crop-243x107"),
    pytest.param("reverse", 1, 2, 243, 107, 3, 0, 3, 1, 0, 0.01, 0.5, id="gray-crop-243x107-reverse"),
    pytest.param("plain", 1, 2, 250, 110, 3, 0, 3, 1, 0, 0.01, 0.5, id="gray-crop-250x110-plain"),
    pytest.param("plain", 3, 2, 256, 112, 3, 1, 2, 1, 0, 0.01, 0.5, id="rgb-plain-subrange-1-2-of-3"),
    pytest.param("seq_rev", 1, 2, 256, 112, 5, 1, 3, 1, 0, 0.01, 0.5, id="gray-subrange-1-3-of-5"),
    pytest.param("reverse", 3, 2, 250, 110, 4, 3, 1, 1, 0, 0.01, 0.5, id="rgb-subrange-3-1-of-4"),
    pytest.param("seq_rev", 1, 2, 256, 112, 16, 0, 16, 2, 0, 0.01, 0.5, id="gray-16-pairs-pipelined"),
    pytest.param("seq_rev", 1, 2, 256, 112, 3, 0, 3, 1, 1, 0.01, 0.5, id="gray-fused-contract"),
    pytest.param("reverse", 3, 2, 256, 112, 2, 0, 2, 1, 1, 0.01, 0.5, id="rgb-fused-contract"),
    pytest.param("plain", 1, 2, 256, 112, 3, 0, 3, 1, 1, 0.01, 0.5, id="gray-plain-fused-contract"),
    pytest.param("seq_rev", 1, 2, 256, 112, 3, 0, 3, 1, 0, 0.0, 0.0, id="gray-alpha0-beta0"),
]


@pytest.mark.parametrize("kind,noc,opp,w,h,n,first,count,pipeline,contract,alpha,beta", FUSED_CASES)
def test_fused_matches_standalone(gpu, kind, noc, opp, w, h, n, first, count, pipeline, contract, alpha, beta):
    fits = [dict(model=model, rounds=rounds, thresh=thresh) for model, rounds, thresh in FUSED_FITS]
    cases.check_fused_matches_standalone(gpu, 6, fits, kind, noc, opp, w, h, n, first, count, pipeline, contract, alpha, beta)


def test_fused_into_device_buffers_on_a_stream(gpu):
    """models_ptr / stats_ptr / out_ptr / stream: the same bytes as the host-array form; stats = NULL and one output alone"""
    w, h, n = 256, 112, 2
    clip = smooth_clip(w, h, 1, n + 1)
    b, devs = run_context(gpu, clip)
    s = gpu.Stream()
    try:
        want_fit = b.global_motion(w, h, rounds=3, thresh=1.0, fb_check=True)
        want = b.motion_compensate(want_fit[0], w, h, thresh=1.0, fb_check=True)
        dm, dst = gpu.Dev(nbytes=n * 48), gpu.Dev(nbytes=n * 24)
        dr, dl = gpu.Dev(nbytes=want[0].nbytes), gpu.Dev(nbytes=want[1].nbytes)
        assert b.global_motion(w, h, rounds=3, thresh=1.0, fb_check=True, models_ptr=dm.ptr, stats_ptr=dst.ptr, stream=s.ptr) is None
        # (the models are read from the device buffer the fit just wrote, on the same stream: no host round trip)
        assert b.motion_compensate(dm.ptr, w, h, thresh=1.0, fb_check=True, out_ptr=(dr.ptr, dl.ptr), stream=s.ptr) is None
        gpu.check(gpu.lib().ofdis_sync(s.ptr))
        assert_same_bits(dm.get((n, 6), np.float64), want_fit[0], "device-buffer form, models")
        assert_same_bits(dst.get((n, 3), np.int64), want_fit[1], "device-buffer form, stats")
        assert_same_bits(dr.get(want[0].shape, _f32), want[0], "device-buffer form, residual")
        assert_same_bits(dl.get(want[1].shape, np.uint8), want[1], "device-buffer form, label")
        dm2 = gpu.Dev(nbytes=n * 48)
        assert b.global_motion(w, h, rounds=3, thresh=1.0, fb_check=True, models_ptr=dm2.ptr, stream=s.ptr) is None
        gpu.check(gpu.lib().ofdis_sync(s.ptr))
        assert_same_bits(dm2.get((n, 6), np.float64), want_fit[0], "stats = NULL")
        res, none = b.motion_compensate(want_fit[0], w, h, thresh=1.0, fb_check=True, label=False)
        assert none is None
        assert_same_bits(res, want[0], "label = NULL")
        none, label = b.motion_compensate(want_fit[0], w, h, thresh=1.0, fb_check=True, residual=False)
        assert none is None
        assert_same_bits(label, want[1], "residual = NULL")
    finally:
        b.close()
        s.close()


# ------------------------------------------------------------------ 4. checks that need a context
@pytest.fixture(scope="module")
def contexts(gpu):
    yield from flag_contexts(gpu, stereo=True)


def _fit_call(gpu, b, first=0, count=3, model=1, rounds=3, thresh=1.0, fb=0, alpha=0.01, beta=0.5, models=True, wo=256, ho=112):
    """host buffers stand in for the device arrays: every call returns before it would launch"""
    m, s = np.zeros((4, 6), np.float64), np.zeros((4, 3), np.int64)
    return gpu.lib().ofdis_batch_global_motion(b.h, first, count, model, rounds, thresh, fb, alpha, beta,
                                               m.ctypes.data if models else None, s.ctypes.data, wo, ho, None)


def _comp_call(gpu, b, first=0, count=3, thresh=1.0, fb=0, alpha=0.01, beta=0.5, models=True, outputs=True, wo=256, ho=112):
    m = np.zeros((4, 6), np.float64)
    r, l = np.zeros((4, 112, 256, 2), _f32), np.zeros((4, 112, 256), np.uint8)
    return gpu.lib().ofdis_batch_motion_compensate(b.h, first, count, m.ctypes.data if models else None, thresh, fb, alpha, beta,
                                                   r.ctypes.data if outputs else None, l.ctypes.data if outputs else None, wo, ho,
                                                   None)


@pytest.mark.parametrize("which", ["stereo", "stereo_lr"])
def test_batch_calls_reject_stereo_contexts(gpu, contexts, which):
    for call in (_fit_call, _comp_call):
        assert call(gpu, contexts[which]) == INVALID
        assert "stereo" in gpu.lib().ofdis_last_error().decode()


@pytest.mark.parametrize("which", ["plain", "seq"])
def test_fb_check_names_the_missing_flag(gpu, contexts, which):
    for call in (_fit_call, _comp_call):
        assert call(gpu, contexts[which], fb=1) == INVALID
        assert "OFDIS_BATCH_REVERSE" in gpu.lib().ofdis_last_error().decode()


COMMON_REJECTS = [dict(models=False)] + RANGE_REJECTS + SIZE_REJECTS + [
    dict(thresh=0.0), dict(thresh=-1.0), dict(thresh=math.nan), dict(thresh=math.inf), dict(fb=2), dict(fb=-1)] + FB_REJECTS
_ids = lambda kw: ",".join(f"{k}={v}" for k, v in kw.items())


@pytest.mark.parametrize("kw", COMMON_REJECTS + [dict(model=-1), dict(model=2), dict(rounds=0), dict(rounds=9), dict(rounds=-1)],
                         ids=_ids)
def test_batch_global_motion_rejects(gpu, contexts, kw):
    assert _fit_call(gpu, contexts["seq_rev"], **kw) == INVALID
    assert gpu.lib().ofdis_last_error()


@pytest.mark.parametrize("kw", COMMON_REJECTS + [dict(outputs=False)], ids=_ids)
def test_batch_motion_compensate_rejects(gpu, contexts, kw):
    assert _comp_call(gpu, contexts["seq_rev"], **kw) == INVALID
    assert gpu.lib().ofdis_last_error()


def test_batch_calls_reject_sides_above_the_limit(gpu, contexts):
    """an original side above OFDIS_GM_MAX_SIDE is named as such (whatever the context's padded size)"""
    for call in (_fit_call, _comp_call):
        for kw in (dict(wo=8193), dict(ho=8193)):
            assert call(gpu, contexts["seq_rev"], **kw) == INVALID
            assert "OFDIS_GM_MAX_SIDE" in gpu.lib().ofdis_last_error().decode()


# ------------------------------------------------------------------ 5. end to end
def _moving_block_pair(w, h, cam, blk, side, at, seed=77):
    """A: a window of a gen_synth texture of (w + 64) x (h + 64); B: the same window displaced by the integer vector `cam`, so
    the background's true model is exactly that translation.  A square of a second texture (side x side at `at` in A) is
    pasted on and moves by the integer vector `blk`.  Returns (A, B, the square in A as a bool map)."""
    bg = gen_synth._texture(np.random.default_rng(seed), h - 64, w - 64)
    fg = gen_synth._texture(np.random.default_rng(seed + 1), side - 128, side - 128)
    assert bg.shape == (h + 64, w + 64) and fg.shape == (side, side)
    to_u8 = lambda t: np.clip(np.rint(t), 0, 255).astype(np.uint8)
    A = to_u8(bg[32:32 + h, 32:32 + w]).copy()
    B = to_u8(bg[32 - cam[1]:32 - cam[1] + h, 32 - cam[0]:32 - cam[0] + w]).copy()
    x0, y0 = at
    A[y0:y0 + side, x0:x0 + side] = to_u8(fg)
    B[y0 + blk[1]:y0 + blk[1] + side, x0 + blk[0]:x0 + blk[0] + side] = to_u8(fg)
    inside = np.zeros((h, w), bool)
    inside[y0:y0 + side, x0:x0 + side] = True
    return A, B, inside


def test_end_to_end_camera_and_moving_block(gpu):
    """A 256x128 gray pair whose background moves by exactly (3, -2) and on which a 70x70 square (15 % of the frame) moves by
    (-5, 4): Batch.global_motion at operating point 2, affine, thresh 1.0, forward-backward test on.  The trimmed fit (rounds =
    3) must be strictly closer to the background's translation than the plain least-squares fit (rounds = 1); more than half of
    the square's pixels eroded by 8 px must be labelled OUTLIER and more than half of the background pixels at least 16 px from
    the square and the border INLIER.
    Measured on an MI355X: translation error 1.4068 px with rounds = 1 and 0.1622 px with rounds = 3 (29312 valid pixels, 15066
    in the last fit); OUTLIER on 1.000 of the eroded square, INLIER on 0.990 of the far background.  The absolute bound below is
    twice the measured rounds = 3 error."""
    from scipy.ndimage import binary_dilation, binary_erosion
    w, h, cam, blk, side, at = 256, 128, (3, -2), (-5, 4), 70, (120, 30)
    A, B, inside = _moving_block_pair(w, h, cam, blk, side, at)
    b, devs = run_context(gpu, np.stack([A, B]), "reverse")
    try:
        fits = {r: b.global_motion(w, h, model=GM_AFFINE, rounds=r, thresh=1.0, fb_check=True) for r in (1, 3)}
        label = b.motion_compensate(fits[3][0], w, h, thresh=1.0, fb_check=True, residual=False)[1][0]
    finally:
        b.close()
    err = {r: max(abs(fits[r][0][0, 0] - cam[0]), abs(fits[r][0][0, 3] - cam[1])) for r in (1, 3)}
    core = binary_erosion(inside, iterations=8)
    far = ~binary_dilation(inside, iterations=16)
    far[:16], far[-16:], far[:, :16], far[:, -16:] = False, False, False, False
    out_share, in_share = (label[core] == GM_OUTLIER).mean(), (label[far] == GM_INLIER).mean()
    print(f"translation error: rounds 1 {err[1]:.4f} px, rounds 3 {err[3]:.4f} px; stats {fits[1][1][0].tolist()} "
          f"{fits[3][1][0].tolist()}; OUTLIER on the eroded square {out_share:.3f}, INLIER on the far background {in_share:.3f}")
    assert core.sum() > 2000 and far.sum() > 5000
    assert err[3] < err[1]
    assert err[3] < 0.33
    assert out_share > 0.5
    assert in_share > 0.5


# ------------------------------------------------------------------ 6. the command-line tool
def test_camera_motion_tool(gpu, tmp_path):
    """tools/camera_motion.py on three PNGs: the CSV holds what Batch.global_motion returns for the same clip, the label PNGs
    what Batch.motion_compensate returns"""
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
    res = subprocess.run([sys.executable, tool, "--rounds", "2", "--thresh", "0.75", "--labels", stem] + paths + [csv],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout, res.stderr)
    b, devs = run_context(gpu, clip)
    try:
        models, stats = b.global_motion(w, h, rounds=2, thresh=0.75, fb_check=True)
        label = b.motion_compensate(models, w, h, thresh=0.75, fb_check=True, residual=False)[1]
    finally:
        b.close()
    rows = [line.split(",") for line in open(csv).read().splitlines()]
    assert len(rows) == n and all(len(r) == 9 for r in rows)
    got_models = np.array([[float(v) for v in r[:6]] for r in rows], np.float64)
    got_stats = np.array([[int(v) for v in r[6:]] for r in rows], np.int64)
    assert_same_bits(got_models, models, "the tool's models")
    assert_same_bits(got_stats, stats, "the tool's stats")
    assert (stats[:, 2] == GM_OK_AFFINE).all() and (stats[:, 1] > 0).all()
    grey = np.array([0, 127, 255], np.uint8)
    for k in range(n):
        assert_same_bits(np.asarray(Image.open(f"{stem}_{k:03d}.png")), grey[label[k]], f"label map {k}")
    res = subprocess.run([sys.executable, tool, "--rounds", "9"] + paths, capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "--rounds" in (res.stderr + res.stdout)
