"""-m gpu: projective video stabilisation (include/ofdis.h: ofdis_camera_path_projective and ofdis_warp_frames_projective on
their own, ofdis_batch_stabilize_projective on an OFDIS_BATCH_SEQUENCE context).

The two kernels are compared bit for bit -- the warps as raw 64-bit patterns, `out` and `inside` as bytes -- with
of_dis_amd/stabilize.py, the header's definition in numpy; the context call bit for bit with its composition
(Batch.projective_motion, capi.camera_path_projective, capi.warp_frames_projective).  Conditions on the generated inputs are
checked on the restatement, never on the kernel under test (those of the models: tests/test_stabilize_projective_ref.py)."""
import math

import numpy as np
import pytest

import launch_hooks
import stab_projective as sp
from of_dis_amd import stabilize
from of_dis_amd.stabilize import (BORDER_CONSTANT, BORDER_REPLICATE, camera_path_projective_ref, camera_path_ref, correction8,
                                  gaussian_weights, smoothed_map8, warp_frames_projective_ref, warp_positions8)
from seq_products import INVALID, RANGE_REJECTS, SIZE_REJECTS, assert_same_bits, flag_contexts, run_context
from test_gpu_stabilize import BATCH_CASES, _uneven_clip
from test_stabilize_projective_ref import E2E, e2e_ideals

pytestmark = pytest.mark.gpu
GM_AFFINE = 1
FRAME_SIZES = [(256, 128), (1, 1)]


# ------------------------------------------------------------------ 1. ofdis_camera_path_projective against the restatement
def _windows(radius):
    ws = [gaussian_weights(radius, max(radius / 3.0, 0.5))]
    if 0 < radius <= 3:
        w = np.random.default_rng(radius).uniform(0.0, 2.0, radius + 1)      # any shape is allowed: a zero inside, a small w_0
        w[-1], w[0] = 0.0, 1e-3
        ws.append(w)
    return ws


@pytest.mark.parametrize("npairs", [1, 2, 7, 300])
@pytest.mark.parametrize("kind", ["smooth", "wild"])
def test_camera_path_matches_the_definition(gpu, npairs, kind):
    m = sp.models8(npairs, kind)
    nonzero = False
    for w, h in FRAME_SIZES:
        hx, hy = stabilize.half_sides(w, h)
        for radius in (0, 1, 3, 64):
            for weights in _windows(radius):
                Q = [smoothed_map8(m, f, weights, hx, hy)[0] for f in range(npairs + 1)]    # (the zoom enters after the walk)
                for zoom in (1.0, 1.25):
                    want = np.array([correction8(q, zoom, hx, hy) for q in Q])
                    assert_same_bits(gpu.camera_path_projective(m, weights, w, h, zoom), want,
                                      f"{npairs} pairs, {kind}, {w}x{h}, radius {radius}, zoom {zoom}, w_0 {weights[0]}")
                    assert np.isfinite(want).all()
                    nonzero |= bool(want[:, 6:].any())
    if npairs == 300:   # conditions on the input, on the restatement: full and truncated windows, breaks, perspective corrections
        reach = sp.reach8(m, gaussian_weights(64, 20.0), 256, 128)
        if kind == "smooth":
            assert reach.max() == 64
        else:
            assert (reach == 0).sum() > 30
        assert nonzero
    if npairs == 7 and kind == "smooth":   # the restatement's own entry point is the loop above
        assert_same_bits(camera_path_projective_ref(m, weights, zoom, w, h), want, "camera_path_projective_ref")


def test_camera_path_on_a_stream_into_a_device_buffer(gpu):
    """the C call with a stream and device pointers, the weights array overwritten right after the call: they travel in the launch"""
    m = sp.models8(7, "smooth")
    s = gpu.Stream()
    try:
        dm, dw = gpu.Dev(m), gpu.Dev(nbytes=8 * 64)
        weights = gaussian_weights(3, 1.5).copy()
        gpu.check(gpu.lib().ofdis_camera_path_projective(dm.ptr, 7, 256, 128, weights.ctypes.data, 3, 1.25, dw.ptr, s.ptr))
        want = camera_path_projective_ref(m, weights, 1.25, 256, 128)
        weights[:] = math.nan
        gpu.check(gpu.lib().ofdis_sync(s.ptr))
        assert_same_bits(dw.get((8, 8), np.float64), want, "on a stream")
        assert want[:, 6:].any()
    finally:
        s.close()


def test_affine_models_give_the_affine_path_to_rounding(gpu):
    """a6 = a7 = 0 through both kernels: g6 = g7 = +0 and g0 .. g5 within 1e-12 * max(1, |warp|) of ofdis_camera_path's"""
    m = np.ascontiguousarray(sp.models8(300, "smooth")[:, :6])
    m8 = np.concatenate([m, np.zeros((300, 2))], axis=1)
    weights = gaussian_weights(64, 20.0)
    a, p = gpu.camera_path(m, weights, 1.25), gpu.camera_path_projective(m8, weights, 256, 128, 1.25)
    assert not np.ascontiguousarray(p[:, 6:]).view(np.uint64).any()
    assert (np.abs(p[:, :6] - a) <= 1e-12 * np.maximum(1.0, np.abs(a))).all(), np.abs(p[:, :6] - a).max()
    assert np.abs(camera_path_ref(m, weights, 1.25)).max() > 1.0


# ------------------------------------------------------------------ 2. ofdis_warp_frames_projective against the restatement
SIZES = [(64, 16), (37, 11), (6, 5), (1, 1)]
NFRAMES = sp.NFRAMES


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("border", [BORDER_CONSTANT, BORDER_REPLICATE], ids=["constant", "replicate"])
def test_warp_frames_matches_the_definition(gpu, noc, w, h, border, which):
    frames, warps = sp.warp_case(w, h, noc, which)
    want = warp_frames_projective_ref(frames, warps, border)
    got = gpu.warp_frames_projective(frames, warps, border)
    assert_same_bits(got[0], want[0], f"noc {noc}, {w}x{h}, border {border}, set {which}, out")
    assert_same_bits(got[1], want[1], f"noc {noc}, {w}x{h}, border {border}, set {which}, inside")
    only, none = gpu.warp_frames_projective(frames, warps, border, inside=False)
    assert none is None
    assert_same_bits(only, want[0], "inside = NULL")
    if which == "b":
        return
    # the header's consequences and the conditions on the input, on the restatement the kernel was just compared with
    assert np.array_equal(want[0][0], frames[0]) and (want[1][0] == 1).all()
    assert not want[1][6:9].any()
    if border == BORDER_CONSTANT:
        assert not want[0][6:9].any()
    front = warp_positions8(warps[5], w, h)[2]
    assert not want[1][5][~front].any()
    if w > 3 and h > 2:
        assert np.array_equal(want[0][1][2:, :w - 3], frames[1][:h - 2, 3:]) and want[1][1].sum() == (h - 2) * (w - 3)
        assert 0 < want[1][5].sum() < w * h and not front.all()          # the crossing: part of the frame, not all of it
        assert (want[0][4] != warp_frames_projective_ref(frames[4:5], np.zeros((1, 8)), border)[0][0]).any()   # the keystone moves pixels


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("border", [BORDER_CONSTANT, BORDER_REPLICATE], ids=["constant", "replicate"])
def test_without_perspective_terms_the_bytes_are_the_affine_warp_s(gpu, noc, w, h, border):
    frames, warps = sp.warp_case(w, h, noc, "a")
    g = warps.copy()
    g[:, 6:] = 0.0
    want = gpu.warp_frames(frames, np.ascontiguousarray(g[:, :6]), border)
    got = gpu.warp_frames_projective(frames, g, border)
    assert_same_bits(got[0], want[0], f"noc {noc}, {w}x{h}, border {border}, out")
    assert_same_bits(got[1], want[1], f"noc {noc}, {w}x{h}, border {border}, inside")


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", [(64, 16), (37, 11), (6, 5)], ids=["64x16", "37x11", "6x5"])
def test_unaligned_outputs_take_byte_stores_with_the_same_bytes(gpu, noc, w, h):
    """out and inside one byte into their buffers: the definition's bytes again, and the guard bytes around both stay"""
    guard = 257
    frames, warps = sp.warp_case(w, h, noc, "a")
    want = warp_frames_projective_ref(frames, warps, BORDER_REPLICATE)
    obytes, ibytes = frames.nbytes, NFRAMES * h * w
    df, dw = gpu.Dev(frames), gpu.Dev(warps)
    for off in (guard, 256):
        do = gpu.Dev(np.full(obytes + 2 * guard, 0xAB, np.uint8))
        di = gpu.Dev(np.full(ibytes + 2 * guard, 0xAB, np.uint8))
        gpu.check(gpu.lib().ofdis_warp_frames_projective(df.ptr, dw.ptr, do.ptr + off, di.ptr + off, NFRAMES, w, h, noc,
                                                         BORDER_REPLICATE, None))
        gpu.check(gpu.lib().ofdis_sync(None))
        o, i = do.get((obytes + 2 * guard,), np.uint8), di.get((ibytes + 2 * guard,), np.uint8)
        for buf, n in ((o, obytes), (i, ibytes)):
            assert (buf[:off] == 0xAB).all() and (buf[off + n:] == 0xAB).all(), off
        assert_same_bits(o[off:off + obytes].reshape(frames.shape), want[0], f"out at offset {off}")
        assert_same_bits(i[off:off + ibytes].reshape(NFRAMES, h, w), want[1], f"inside at offset {off}")


@pytest.mark.parametrize("limit", [8, 3])
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", [(64, 16), (37, 11)], ids=["64x16", "37x11"])
def test_warp_frames_in_chunks(gpu, noc, w, h, limit):
    """the launcher's second chunk: the test library's launcher with QUAD_MAX_BLOCKS lowered to 8 (chunks of 8 and 3 frames) and
    to 3 (four chunks), the same bytes"""
    hook = launch_hooks.hooks().ofdis_test_launch_warp_frames_projective
    frames, warps = sp.warp_case(w, h, noc, "a")
    want = warp_frames_projective_ref(frames, warps, BORDER_CONSTANT)
    df, dw = gpu.Dev(frames), gpu.Dev(warps)
    do, di = gpu.Dev(np.full(frames.nbytes, 0xAB, np.uint8)), gpu.Dev(np.full(NFRAMES * h * w, 0xAB, np.uint8))
    with launch_hooks.launch_limits(quad_max_blocks=limit):
        walk = launch_hooks.chunk_walk(NFRAMES, w, h)[1]
        assert len(walk) >= 2 and sum(n for _, n, _ in walk) == NFRAMES, walk
        assert hook(df.ptr, dw.ptr, do.ptr, di.ptr, NFRAMES, w, h, noc, 0, None) == 0
        gpu.check(gpu.lib().ofdis_sync(None))
    assert_same_bits(do.get(frames.shape, np.uint8), want[0], f"chunks {walk}, out")
    assert_same_bits(di.get((NFRAMES, h, w), np.uint8), want[1], f"chunks {walk}, inside")


# ------------------------------------------------------------------ 3. ofdis_batch_stabilize_projective against its composition
@pytest.mark.parametrize("noc,w,h,n,first,count,pipeline,contract", BATCH_CASES)
def test_batch_stabilize_projective_matches_the_three_calls(gpu, noc, w, h, n, first, count, pipeline, contract):
    clip = _uneven_clip(w, h, noc, n + 1)
    weights, zoom = gaussian_weights(2, 1.0), 1.05
    b, (d,) = run_context(gpu, clip, "seq_rev", 2, contract, pipeline)
    got, models = {}, {}
    try:
        bytes_before = b.device_bytes()
        for fb in (0, 1):
            border = BORDER_REPLICATE if fb else BORDER_CONSTANT
            got[fb] = b.stabilize_projective(d.ptr, w, h, weights, zoom=zoom, border=border, rounds=3, thresh=1.0, fb_check=fb,
                                             first=first, count=count, inside=True)
            if fb == 0:   # the models and warps belong to the context: allocated by the first call, counted from then on
                grown = b.device_bytes() - bytes_before
                assert grown >= (2 * n + 1) * 64
        assert b.device_bytes() - bytes_before == grown
        for fb in (0, 1):
            models[fb] = b.projective_motion(w, h, rounds=3, thresh=1.0, fb_check=fb, first=first, count=count)[0]
    finally:
        b.close()
    for fb in (0, 1):
        border = BORDER_REPLICATE if fb else BORDER_CONSTANT
        warps = gpu.camera_path_projective(models[fb], weights, w, h, zoom)
        out, inside = gpu.warp_frames_projective(clip[first:first + count + 1], warps, border)
        assert_same_bits(got[fb][2], warps, f"fb_check {fb}, warps")
        assert_same_bits(got[fb][0], out, f"fb_check {fb}, out")
        assert_same_bits(got[fb][1], inside, f"fb_check {fb}, inside")
        # ... and the composition is the definition's (conditions on the input: something was corrected, perspective terms too)
        assert_same_bits(warps, camera_path_projective_ref(models[fb], weights, zoom, w, h), f"fb_check {fb}, warps vs the definition")
        assert np.abs(warps[1:-1, [0, 3]]).max() > 0.05 and warps[1:-1, 6:].any() and not warps[0, [0, 2, 3, 4, 6, 7]].any()
        assert (out != clip[first:first + count + 1]).any()


def test_batch_stabilize_projective_into_device_buffers_on_a_stream(gpu):
    """out_ptr / inside pointer / warps_ptr / stream: the same bytes as the host-array form; inside = NULL and warps = NULL"""
    w, h, n = 256, 112, 3
    clip = _uneven_clip(w, h, 1, n + 1)
    weights = gaussian_weights(1, 1.0)
    b, (d,) = run_context(gpu, clip)
    s = gpu.Stream()
    try:
        want = b.stabilize_projective(d.ptr, w, h, weights, fb_check=True, inside=True)
        do, di, dw = gpu.Dev(nbytes=want[0].nbytes), gpu.Dev(nbytes=want[1].nbytes), gpu.Dev(nbytes=want[2].nbytes)
        assert b.stabilize_projective(d.ptr, w, h, weights, fb_check=True, out_ptr=do.ptr, inside=di.ptr, warps_ptr=dw.ptr,
                                      stream=s.ptr) is None
        gpu.check(gpu.lib().ofdis_sync(s.ptr))
        assert want[2].shape == (n + 1, 8)
        assert_same_bits(do.get(want[0].shape, np.uint8), want[0], "device-buffer form, out")
        assert_same_bits(di.get(want[1].shape, np.uint8), want[1], "device-buffer form, inside")
        assert_same_bits(dw.get(want[2].shape, np.float64), want[2], "device-buffer form, warps")
        do2 = gpu.Dev(np.full(want[0].nbytes, 0xAB, np.uint8))
        assert b.stabilize_projective(d.ptr, w, h, weights, fb_check=True, out_ptr=do2.ptr, stream=s.ptr) is None
        gpu.check(gpu.lib().ofdis_sync(s.ptr))
        assert_same_bits(do2.get(want[0].shape, np.uint8), want[0], "inside = NULL, warps = NULL")
    finally:
        b.close()
        s.close()


# ------------------------------------------------------------------ 4. checks that need a context
@pytest.fixture(scope="module")
def contexts(gpu):
    yield from flag_contexts(gpu, stereo=True)


def _call(gpu, b, first=0, count=3, rounds=3, thresh=1.0, fb=0, alpha=0.01, beta=0.5, frames=True, out=True, in_place=False,
          weights=True, w0=1.0, radius=2, zoom=1.0, border=0, wo=256, ho=112):
    """host buffers stand in for the device arrays: every call returns before it would launch"""
    fr, o = np.zeros(4 * 256 * 112, np.uint8), np.zeros(4 * 256 * 112, np.uint8)
    wts = np.full(66, w0, np.float64)
    optr = fr.ctypes.data if in_place else (o.ctypes.data if out else None)
    return gpu.lib().ofdis_batch_stabilize_projective(b.h, fr.ctypes.data if frames else None, first, count, rounds, thresh, fb,
                                                      alpha, beta, wts.ctypes.data if weights else None, radius, zoom, border,
                                                      optr, None, None, wo, ho, None)


@pytest.mark.parametrize("which", ["plain", "reverse"])
def test_batch_stabilize_projective_names_the_missing_flag(gpu, contexts, which):
    assert _call(gpu, contexts[which]) == INVALID
    assert "OFDIS_BATCH_SEQUENCE" in gpu.lib().ofdis_last_error().decode()


@pytest.mark.parametrize("which", ["stereo", "stereo_lr"])
def test_batch_stabilize_projective_rejects_stereo_contexts(gpu, contexts, which):
    assert _call(gpu, contexts[which]) == INVALID
    assert "stereo" in gpu.lib().ofdis_last_error().decode()


def test_fb_check_names_the_missing_flag(gpu, contexts):
    assert _call(gpu, contexts["seq"], fb=1) == INVALID
    assert "OFDIS_BATCH_REVERSE" in gpu.lib().ofdis_last_error().decode()


@pytest.mark.parametrize("kw", [
    dict(frames=False), dict(out=False), dict(in_place=True), dict(weights=False)] + RANGE_REJECTS + SIZE_REJECTS + [
    dict(wo=8193), dict(ho=8193),
    dict(rounds=0), dict(rounds=9), dict(thresh=0.0), dict(thresh=math.nan),
    dict(fb=2), dict(fb=-1), dict(alpha=-0.01), dict(beta=math.inf),
    dict(radius=-1), dict(radius=65), dict(w0=0.0), dict(w0=-1.0), dict(w0=math.nan), dict(w0=math.inf),
    dict(zoom=0.5), dict(zoom=16.5), dict(zoom=math.nan), dict(border=-1), dict(border=2),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_batch_stabilize_projective_rejects(gpu, contexts, kw):
    b = contexts["seq_rev"]
    before = b.device_bytes()
    assert _call(gpu, b, **kw) == INVALID
    assert gpu.lib().ofdis_last_error()
    assert b.device_bytes() == before   # a rejected call allocates nothing


# ------------------------------------------------------------------ 5. end to end
def test_end_to_end_a_jittered_rotation_is_smoothed_at_the_corners(gpu):
    """25 gray frames of 256x128 from a camera that only rotates (focal length 150 px): a pan of 0.5 degrees per frame plus
    N(0, 1 / 1 / 0.5 degrees) of pan / tilt / roll per frame (seed 1), rendered by bilinear sampling of one gen_synth texture under
    the homographies C_f.  Batch.stabilize_projective at operating point 2, 3 rounds, thresh 1.0, forward-backward test on,
    Gaussian window of radius 4 and sigma 2, zoom 1; Batch.stabilize (affine) on the same context beside it.
    The metric is the roughness (RMS second difference over the frames) of the four frame corners' positions in the stabilised
    frames, inv(H(g_f)) C_f applied to the corners, over frames 4 .. 20, as a share of the input's.  Preconditions, on the
    restatement fed the true models C_{f+1} C_f^-1 (tests/test_stabilize_projective_ref.py has them on the CPU as well): the
    projective share is below 0.15 (0.093), the affine share with the least-squares affine parts above 0.30 (0.373), every
    pair usable.  Asserted: the share from the ESTIMATED projective models is below 0.19 -- the geometric mean of twice the
    projective ideal and half the affine one -- and below the share Batch.stabilize reaches.
    Measured on an MI355X: projective 0.1005 of the input's roughness (with the true models 0.0926), affine 0.4064 (with the
    least-squares affine parts of the true motion 0.3725); the largest difference between an estimated and a true warp
    translation is 0.0405 px; the largest model error is 0.0694 px in the translation and 1.42e-05 in a6 / a7 (true values up to
    3.03e-04); `inside` on 0.9755 of the pixels.  The flow at operating point 2 follows this motion (up to 13.6 px at the
    corners): pan and jitter are the ones first chosen."""
    w, h, n = E2E["w"], E2E["h"], E2E["n"]
    C, true, ideal_proj, ideal_aff = e2e_ideals(**E2E)
    hx, hy = stabilize.half_sides(w, h)
    assert ideal_proj < 0.15 and ideal_aff > 0.30 and all(stabilize.pair_map8(m, hx, hy)[1] for m in true)
    clip = sp.rotating_clip(w, h, n, E2E["fl"], E2E["pan_deg"], E2E["jitter_deg"], E2E["seed"])[0]
    weights = gaussian_weights(4, 2.0)
    true_warps = camera_path_projective_ref(true, weights, 1.0, w, h)
    b, (d,) = run_context(gpu, clip)
    try:
        out, inside, warps = b.stabilize_projective(d.ptr, w, h, weights, zoom=1.0, border=BORDER_CONSTANT, rounds=3, thresh=1.0,
                                                    fb_check=True, inside=True)
        affine = b.stabilize(d.ptr, w, h, weights, zoom=1.0, border=BORDER_CONSTANT, model=GM_AFFINE, rounds=3, thresh=1.0,
                             fb_check=True, inside=True)[2]
        models = b.projective_motion(w, h, rounds=3, thresh=1.0, fb_check=True)[0]
    finally:
        b.close()
    share, share_affine = sp.corner_share(warps, C, w, h), sp.corner_share(affine, C, w, h)
    worst = np.abs(warps[:, [0, 3]] - true_warps[:, [0, 3]]).max()
    print(f"corner roughness as a share of the input's: projective {share:.4f} (with the true models {ideal_proj:.4f}), affine "
          f"{share_affine:.4f} (with the least-squares affine parts of the true motion {ideal_aff:.4f}); largest difference "
          f"between an estimated and a true warp translation {worst:.4f} px; largest model error: translation "
          f"{np.abs(models[:, [0, 3]] - true[:, [0, 3]]).max():.4f} px, a6 / a7 {np.abs(models[:, 6:] - true[:, 6:]).max():.2e} "
          f"(true up to {np.abs(true[:, 6:]).max():.2e}); inside on {inside.mean():.4f} of the pixels")
    assert out.shape == clip.shape and np.array_equal(out[0], clip[0]) and np.array_equal(out[-1], clip[-1])
    assert share < 0.19, share
    assert share < share_affine, (share, share_affine)


# ------------------------------------------------------------------ 6. the command-line tool
def test_stabilize_frames_tool(gpu, tmp_path):
    """tools/stabilize_frames.py --model projective on five PNGs: the files and the CSV (8 columns) hold what
    Batch.stabilize_projective returns for the clip; without --model they hold what Batch.stabilize returns"""
    import os
    import subprocess
    import sys
    from PIL import Image
    w, h, n = 250, 107, 4
    clip = _uneven_clip(w, h, 1, n + 1)
    paths = []
    for k, f in enumerate(clip):
        paths.append(str(tmp_path / f"f{k}.png"))
        Image.fromarray(f).save(paths[-1])
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "stabilize_frames.py")
    common = ["--radius", "2", "--sigma", "1.5", "--zoom", "1.1", "--border", "replicate"]
    b, (d,) = run_context(gpu, clip)
    try:
        want = {"projective": b.stabilize_projective(d.ptr, w, h, gaussian_weights(2, 1.5), zoom=1.1, border=BORDER_REPLICATE,
                                                     fb_check=True),
                "affine": b.stabilize(d.ptr, w, h, gaussian_weights(2, 1.5), zoom=1.1, border=BORDER_REPLICATE, fb_check=True)}
    finally:
        b.close()
    for model, flags, columns in (("projective", ["--model", "projective"], 8), ("affine", [], 6)):
        stem = str(tmp_path / f"stab_{model}")
        res = subprocess.run([sys.executable, tool] + flags + common + paths + [stem], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, (res.stdout, res.stderr)
        got = np.stack([np.asarray(Image.open(f"{stem}_{k:03d}.png")) for k in range(n + 1)])
        assert_same_bits(got, want[model][0], f"{model}: the tool's files")
        rows = [line.split(",") for line in open(stem + ".csv").read().splitlines()]
        assert len(rows) == n + 1 and all(len(r) == columns for r in rows)
        assert_same_bits(np.array([[float(v) for v in r] for r in rows], np.float64), want[model][2], f"{model}: the tool's warps")
    assert want["projective"][2][:, 6:].any()
    res = subprocess.run([sys.executable, tool, "--model", "homography"] + paths + [stem], capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "--model" in (res.stderr + res.stdout)
