"""-m gpu: video stabilisation (include/ofdis.h: ofdis_camera_path and ofdis_warp_frames on their own, ofdis_batch_stabilize on
an OFDIS_BATCH_SEQUENCE context).

The two kernels are compared bit for bit -- the warps as raw 64-bit patterns, `out` and `inside` as bytes -- with
of_dis_amd/stabilize.py, the header's definition in numpy; the context call bit for bit with its composition
(Batch.global_motion, capi.camera_path, capi.warp_frames).  Conditions on the generated inputs are checked on the restatement,
never on the kernel under test."""
import functools
import math

import numpy as np
import pytest

import gen_synth
from of_dis_amd import stabilize
from of_dis_amd.stabilize import (BORDER_CONSTANT, BORDER_REPLICATE, camera_path_ref, gaussian_weights, smoothed_map,
                                  warp_frames_ref)
from seq_products import INVALID, RANGE_REJECTS, SIZE_REJECTS, assert_same_bits, flag_contexts, run_context, smooth_clip

pytestmark = pytest.mark.gpu
GM_AFFINE = 1


# ------------------------------------------------------------------ 1. ofdis_camera_path against the restatement
@functools.lru_cache(maxsize=None)
def _models(npairs, kind):
    """"smooth": small random affines (translations of a few pixels, linear parts within 2 % of the identity).  "wild": the
    same with NaN, infinities, huge finite translations, singular, mirrored and inflated linear parts at random places."""
    rng = np.random.default_rng(1000 + npairs + (7 if kind == "wild" else 0))
    m = rng.normal(0.0, 1.0, (npairs, 6)) * np.array([3.0, 0.02, 0.02, 3.0, 0.02, 0.02])
    if kind == "wild":
        pick = rng.random(npairs)
        col = rng.integers(0, 6, npairs)
        rows = np.arange(npairs)
        for lo, hi, value in ((0.00, 0.03, math.nan), (0.03, 0.06, math.inf), (0.06, 0.09, -math.inf), (0.09, 0.13, 1.7e308),
                              (0.13, 0.16, -1e300)):
            sel = (pick >= lo) & (pick < hi)
            m[rows[sel], col[sel]] = value
        for lo, hi, lin in ((0.16, 0.19, (-1.0, 0.0, 0.0, -1.0)),      # A = 0
                            (0.19, 0.22, (-2.0, 0.0, 0.0, 0.0)),       # a mirror, det = -1
                            (0.22, 0.25, (1.5, 0.0, 0.0, 1.0)),        # det = 5
                            (0.25, 0.28, (0.0, 1.0, 0.75, 0.0)),       # det = 0.25 exactly: usable
                            (0.28, 0.31, (1.0, 0.0, 0.0, 1.0))):       # det = 4 exactly: usable
            sel = (pick >= lo) & (pick < hi)
            m[sel, 1], m[sel, 2], m[sel, 4], m[sel, 5] = lin
    return m


def _windows(radius):
    rng = np.random.default_rng(radius)
    ws = [gaussian_weights(radius, max(radius / 3.0, 0.5))]
    if radius:
        w = rng.uniform(0.0, 2.0, radius + 1)      # any shape is allowed: zeros inside, a small w_0
        w[rng.random(radius + 1) < 0.3] = 0.0
        w[0] = 1e-3
        ws.append(w)
    return ws


@pytest.mark.parametrize("npairs", [1, 2, 7, 300])
@pytest.mark.parametrize("kind", ["smooth", "wild"])
def test_camera_path_matches_the_definition(gpu, npairs, kind):
    m = _models(npairs, kind)
    for radius in (0, 1, 3, 64):
        for weights in _windows(radius):
            for zoom in (1.0, 1.25):
                want = camera_path_ref(m, weights, zoom)
                assert_same_bits(gpu.camera_path(m, weights, zoom), want,
                                  f"{npairs} pairs, {kind}, radius {radius}, zoom {zoom}, w_0 {weights[0]}")
                assert np.isfinite(want).all()
    if npairs == 300:   # conditions on the input, on the restatement: full and truncated windows, breaks, corrections that matter
        w = gaussian_weights(64, 20.0)
        reach = np.array([smoothed_map(m, f, w)[1] for f in range(npairs + 1)])
        if kind == "smooth":
            assert reach.max() == 64 and (reach == 64).sum() == 301 - 128 and np.abs(camera_path_ref(m, w)).max() > 1.0
        else:
            assert (reach == 0).sum() > 30 and 3 < reach.max() < 64


def test_camera_path_on_a_stream_into_a_device_buffer(gpu):
    """the C call with a stream and device pointers, the weights array freed right after the call: they travel in the launch"""
    m = _models(7, "smooth")
    s = gpu.Stream()
    try:
        dm, dw = gpu.Dev(m), gpu.Dev(nbytes=8 * 48)
        weights = gaussian_weights(3, 1.5).copy()
        gpu.check(gpu.lib().ofdis_camera_path(dm.ptr, 7, weights.ctypes.data, 3, 1.25, dw.ptr, s.ptr))
        want = camera_path_ref(m, weights, 1.25)
        weights[:] = math.nan
        gpu.check(gpu.lib().ofdis_sync(s.ptr))
        assert_same_bits(dw.get((8, 6), np.float64), want, "on a stream")
    finally:
        s.close()


# ------------------------------------------------------------------ 2. ofdis_warp_frames against the restatement
SIZES = [(64, 16), (37, 11), (6, 5), (1, 1)]
NFRAMES = 11   # more frames than XCDs in one launch, with a padded last group


@functools.lru_cache(maxsize=None)
def _warp_case(w, h, noc):
    """11 random frames, one warp each: zero, an integer translation, a half-pixel translation, a rotation by 3 degrees with zoom
    1.1, a NaN warp, a warp that throws every sample outside, an infinite one, and four random small affines"""
    rng = np.random.default_rng(w * 100 + h * 10 + noc)
    frames = rng.integers(0, 256, (NFRAMES, h, w) + ((3,) if noc == 3 else ()), dtype=np.uint8)
    warps = np.zeros((NFRAMES, 6))
    warps[1, [0, 3]] = 3.0, -2.0
    warps[2, [0, 3]] = 0.5, -0.5
    c, s = math.cos(math.radians(3.0)) / 1.1, math.sin(math.radians(3.0)) / 1.1
    warps[3] = 0.3, c - 1.0, -s, -0.2, s, c - 1.0
    warps[4, 2] = math.nan
    warps[5, [0, 3]] = 3.0 * w + 5, -2.0 * h - 7
    warps[6, [0, 4]] = math.inf, -math.inf
    warps[7:] = rng.normal(0.0, 1.0, (NFRAMES - 7, 6)) * np.array([2.0, 0.05, 0.05, 2.0, 0.05, 0.05])
    return frames, warps


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("border", [BORDER_CONSTANT, BORDER_REPLICATE], ids=["constant", "replicate"])
def test_warp_frames_matches_the_definition(gpu, noc, w, h, border):
    frames, warps = _warp_case(w, h, noc)
    want = warp_frames_ref(frames, warps, border)
    got = gpu.warp_frames(frames, warps, border)
    assert_same_bits(got[0], want[0], f"noc {noc}, {w}x{h}, border {border}, out")
    assert_same_bits(got[1], want[1], f"noc {noc}, {w}x{h}, border {border}, inside")
    # inside = NULL writes the same out
    only, none = gpu.warp_frames(frames, warps, border, inside=False)
    assert none is None
    assert_same_bits(only, want[0], "inside = NULL")
    # the header's consequences, on the restatement the kernel was just compared with
    assert np.array_equal(want[0][0], frames[0]) and (want[1][0] == 1).all()
    assert not want[1][4:7].any()
    if border == BORDER_CONSTANT:
        assert not want[0][4:7].any()
    if w > 3 and h > 2:
        assert np.array_equal(want[0][1][2:, :w - 3], frames[1][:h - 2, 3:])
        assert (want[1][1][2:, :w - 3] == 1).all() and want[1][1].sum() == (h - 2) * (w - 3)
        if border == BORDER_CONSTANT:
            assert not want[0][1][:2].any() and not want[0][1][:, w - 3:].any()
        assert 0 < want[1][3].sum() < w * h or w * h < 64      # the rotation leaves part of the frame uncovered


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", [(64, 16), (37, 11), (6, 5)], ids=["64x16", "37x11", "6x5"])
def test_unaligned_outputs_take_byte_stores_with_the_same_bytes(gpu, noc, w, h):
    """out and inside one byte into their buffers: the definition's bytes again, and the guard bytes around both stay"""
    guard = 257   # (the arrays start at byte 257 of their buffers: 1 mod 4)
    frames, warps = _warp_case(w, h, noc)
    want = warp_frames_ref(frames, warps, BORDER_REPLICATE)
    obytes, ibytes = frames.nbytes, NFRAMES * h * w
    df, dw = gpu.Dev(frames), gpu.Dev(warps)
    for off in (guard, 256):   # (and the aligned call with the same guards)
        do = gpu.Dev(np.full(obytes + 2 * guard, 0xAB, np.uint8))
        di = gpu.Dev(np.full(ibytes + 2 * guard, 0xAB, np.uint8))
        gpu.check(gpu.lib().ofdis_warp_frames(df.ptr, dw.ptr, do.ptr + off, di.ptr + off, NFRAMES, w, h, noc, BORDER_REPLICATE,
                                              None))
        gpu.check(gpu.lib().ofdis_sync(None))
        o, i = do.get((obytes + 2 * guard,), np.uint8), di.get((ibytes + 2 * guard,), np.uint8)
        for buf, n in ((o, obytes), (i, ibytes)):
            assert (buf[:off] == 0xAB).all() and (buf[off + n:] == 0xAB).all(), off
        assert_same_bits(o[off:off + obytes].reshape(frames.shape), want[0], f"out at offset {off}")
        assert_same_bits(i[off:off + ibytes].reshape(NFRAMES, h, w), want[1], f"inside at offset {off}")


# ------------------------------------------------------------------ 3. ofdis_batch_stabilize against its composition
def _uneven_clip(w, h, noc, nframes):
    """nframes (at most 6) frames of one scene in UNEVEN motion: gen_synth's texture displaced by 0, 1, 3, 4, 6, 7 times 0.1 of
    its flow (up to 12 px), so the pairs move by up to 1.2 and 2.4 px in turn and a smoothed path differs from the camera's"""
    return smooth_clip(w, h, noc, nframes, step=0.1, walk=(0, 1, 3, 4, 6, 7))


# (noc, w, h, n pairs, first, count, pipeline, contract)
BATCH_CASES = [
    pytest.param(1, 256, 112, 5, 1, 3, 1, 0, id="gray-subrange-1-3-of-5"),
    pytest.param(3, 256, 112, 5, 1, 3, 1, 0, id="rgb-subrange-1-3-of-5"),
    pytest.param(1, 256, 112, 5, 1, 3, 1, 1, id="gray-fused-contract"),
    pytest.param(3, 256, 112, 5, 1, 3, 1, 1, id="rgb-fused-contract"),
    pytest.param(1, 256, 112, 5, 1, 3, 2, 0, id="gray-pipelined"),
    pytest.param(1, 250, 110, 5, 0, 5, 1, 0, id="gray-crop-250x110"),
    pytest.param(3, 250, 110, 5, 1, 3, 2, 1, id="rgb-crop-pipelined-fused-contract"),
]


@pytest.mark.parametrize("noc,w,h,n,first,count,pipeline,contract", BATCH_CASES)
def test_batch_stabilize_matches_the_three_calls(gpu, noc, w, h, n, first, count, pipeline, contract):
    clip = _uneven_clip(w, h, noc, n + 1)
    weights, zoom = gaussian_weights(2, 1.0), 1.05
    b, (d,) = run_context(gpu, clip, "seq_rev", 2, contract, pipeline)
    got, models = {}, {}
    try:
        bytes_before = b.device_bytes()
        for fb in (0, 1):
            border = BORDER_REPLICATE if fb else BORDER_CONSTANT
            got[fb] = b.stabilize(d.ptr, w, h, weights, zoom=zoom, border=border, model=GM_AFFINE, rounds=3, thresh=1.0,
                                  fb_check=fb, first=first, count=count, inside=True)
            if fb == 0:   # the models and warps belong to the context: allocated by the first call, counted from then on
                grown = b.device_bytes() - bytes_before
                assert grown >= (2 * n + 1) * 48
        assert b.device_bytes() - bytes_before == grown
        for fb in (0, 1):
            models[fb] = b.global_motion(w, h, model=GM_AFFINE, rounds=3, thresh=1.0, fb_check=fb, first=first, count=count)[0]
    finally:
        b.close()
    for fb in (0, 1):
        border = BORDER_REPLICATE if fb else BORDER_CONSTANT
        warps = gpu.camera_path(models[fb], weights, zoom)
        out, inside = gpu.warp_frames(clip[first:first + count + 1], warps, border)
        assert_same_bits(got[fb][2], warps, f"fb_check {fb}, warps")
        assert_same_bits(got[fb][0], out, f"fb_check {fb}, out")
        assert_same_bits(got[fb][1], inside, f"fb_check {fb}, inside")
        # ... and the composition is the definition's (conditions on the input: something was corrected, something uncovered)
        assert_same_bits(warps, camera_path_ref(models[fb], weights, zoom), f"fb_check {fb}, warps vs the definition")
        assert np.abs(warps[1:-1, [0, 3]]).max() > 0.05 and not warps[0, [0, 2, 3, 4]].any()
        assert (out != clip[first:first + count + 1]).any()


def test_batch_stabilize_into_device_buffers_on_a_stream(gpu):
    """out_ptr / inside pointer / warps_ptr / stream: the same bytes as the host-array form; inside = NULL and warps = NULL"""
    w, h, n = 256, 112, 3
    clip = _uneven_clip(w, h, 1, n + 1)
    weights = gaussian_weights(1, 1.0)
    b, (d,) = run_context(gpu, clip)
    s = gpu.Stream()
    try:
        want = b.stabilize(d.ptr, w, h, weights, fb_check=True, inside=True)
        do, di, dw = gpu.Dev(nbytes=want[0].nbytes), gpu.Dev(nbytes=want[1].nbytes), gpu.Dev(nbytes=want[2].nbytes)
        assert b.stabilize(d.ptr, w, h, weights, fb_check=True, out_ptr=do.ptr, inside=di.ptr, warps_ptr=dw.ptr, stream=s.ptr) is None
        gpu.check(gpu.lib().ofdis_sync(s.ptr))
        assert_same_bits(do.get(want[0].shape, np.uint8), want[0], "device-buffer form, out")
        assert_same_bits(di.get(want[1].shape, np.uint8), want[1], "device-buffer form, inside")
        assert_same_bits(dw.get(want[2].shape, np.float64), want[2], "device-buffer form, warps")
        do2 = gpu.Dev(np.full(want[0].nbytes, 0xAB, np.uint8))
        assert b.stabilize(d.ptr, w, h, weights, fb_check=True, out_ptr=do2.ptr, stream=s.ptr) is None
        gpu.check(gpu.lib().ofdis_sync(s.ptr))
        assert_same_bits(do2.get(want[0].shape, np.uint8), want[0], "inside = NULL, warps = NULL")
    finally:
        b.close()
        s.close()


# ------------------------------------------------------------------ 4. checks that need a context
@pytest.fixture(scope="module")
def contexts(gpu):
    yield from flag_contexts(gpu, stereo=True)


def _call(gpu, b, first=0, count=3, model=1, rounds=3, thresh=1.0, fb=0, alpha=0.01, beta=0.5, frames=True, out=True,
          in_place=False, weights=True, w0=1.0, radius=2, zoom=1.0, border=0, wo=256, ho=112):
    """host buffers stand in for the device arrays: every call returns before it would launch"""
    fr, o = np.zeros(4 * 256 * 112, np.uint8), np.zeros(4 * 256 * 112, np.uint8)
    wts = np.full(66, w0, np.float64)
    optr = fr.ctypes.data if in_place else (o.ctypes.data if out else None)
    return gpu.lib().ofdis_batch_stabilize(b.h, fr.ctypes.data if frames else None, first, count, model, rounds, thresh, fb, alpha,
                                           beta, wts.ctypes.data if weights else None, radius, zoom, border, optr, None, None, wo,
                                           ho, None)


@pytest.mark.parametrize("which", ["plain", "reverse"])
def test_batch_stabilize_names_the_missing_flag(gpu, contexts, which):
    assert _call(gpu, contexts[which]) == INVALID
    assert "OFDIS_BATCH_SEQUENCE" in gpu.lib().ofdis_last_error().decode()


@pytest.mark.parametrize("which", ["stereo", "stereo_lr"])
def test_batch_stabilize_rejects_stereo_contexts(gpu, contexts, which):
    assert _call(gpu, contexts[which]) == INVALID
    assert "stereo" in gpu.lib().ofdis_last_error().decode()


def test_fb_check_names_the_missing_flag(gpu, contexts):
    assert _call(gpu, contexts["seq"], fb=1) == INVALID
    assert "OFDIS_BATCH_REVERSE" in gpu.lib().ofdis_last_error().decode()


@pytest.mark.parametrize("kw", [
    dict(frames=False), dict(out=False), dict(in_place=True), dict(weights=False)] + RANGE_REJECTS + SIZE_REJECTS + [
    dict(wo=8193), dict(ho=8193),
    dict(model=-1), dict(model=2), dict(rounds=0), dict(rounds=9), dict(thresh=0.0), dict(thresh=math.nan),
    dict(fb=2), dict(fb=-1), dict(alpha=-0.01), dict(beta=math.inf),
    dict(radius=-1), dict(radius=65), dict(w0=0.0), dict(w0=-1.0), dict(w0=math.nan), dict(w0=math.inf),
    dict(zoom=0.5), dict(zoom=16.5), dict(zoom=math.nan), dict(border=-1), dict(border=2),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_batch_stabilize_rejects(gpu, contexts, kw):
    b = contexts["seq_rev"]
    before = b.device_bytes()
    assert _call(gpu, b, **kw) == INVALID
    assert gpu.lib().ofdis_last_error()
    assert b.device_bytes() == before   # a rejected call allocates nothing


# ------------------------------------------------------------------ 5. end to end
JITTER_SEED = 1


def _roughness(pos):
    """the RMS second difference of a position sequence [n][2] over the frames"""
    d = pos[2:] - 2.0 * pos[1:-1] + pos[:-2]
    return float(np.sqrt((d * d).sum(axis=1).mean()))


def _jittered_clip(w, h, n, seed=JITTER_SEED):
    """n frames cut from ONE gen_synth texture at the integer window positions pos_f = f * (1, 0) + jitter_f, jitter_f drawn
    from {-1, 0, 1}^2 and jitter_0 = 0: frame f shows texture pixel (x, y) + pos_f at (x, y).  A scene point therefore moves by
    -(pos_{f+1} - pos_f) from frame f to f + 1: the true model of pair f is exactly that translation, at most 3 px."""
    rng = np.random.default_rng(seed)
    jitter = rng.integers(-1, 2, (n, 2))
    jitter[0] = 0
    pos = np.arange(n)[:, None] * np.array([1, 0]) + jitter
    tex = gen_synth._texture(np.random.default_rng(77), h - 64, w - 64)     # (h + 64, w + 64): a margin of 32 px on every side
    assert tex.shape == (h + 64, w + 64) and pos.min() >= -32 and pos.max() <= 32
    u8 = np.clip(np.rint(tex), 0, 255).astype(np.uint8)
    clip = np.stack([u8[32 + py:32 + py + h, 32 + px:32 + px + w] for px, py in pos])
    return np.ascontiguousarray(clip), pos.astype(np.float64)


def test_end_to_end_a_jittered_pan_is_smoothed(gpu):
    """25 gray frames of 256x128 cut from one texture at window positions that pan by (1, 0) per frame plus a jitter from
    {-1, 0, 1}^2 (seed 1; the true per-pair models are exact translations of at most 3 px): Batch.stabilize at operating point
    2, affine, 3 rounds, thresh 1.0, forward-backward test on, Gaussian window of radius 4 and sigma 2, zoom 1.
    The metric is the roughness, the RMS second difference of a position sequence over the frames.  Stabilised frame f shows
    out_f(x) = I_f(x + b) with b = (b0, b3) of warp f, i.e. the texture window at pos_f + b: that is the stabilised position.
    (The flow of a pair, and so its model, is MINUS the step of the window position; with the model read as the window's own
    step the same quantity is pos_f - b.)  Asserted: the stabilised positions have less than 0.25 of the input's roughness,
    and -- a precondition on the input, not on the code under test -- the same ratio from camera_path_ref fed the true
    translations is below 0.1 (this seed: 0.054; the truncated windows of the first and last four frames are what is left).
    Measured on an MI355X: input roughness 3.5139 px, stabilised / input 0.0544 (with the true models 0.0540); the largest
    difference between an estimated and a true warp translation is 0.0160 px; `inside` on 0.9872 of the pixels."""
    w, h, n = 256, 128, 25
    clip, pos = _jittered_clip(w, h, n)
    true = np.zeros((n - 1, 6))
    true[:, [0, 3]] = -(pos[1:] - pos[:-1])
    assert np.abs(true).max() <= 3.0
    weights = gaussian_weights(4, 2.0)
    true_warps = camera_path_ref(true, weights, 1.0)
    rough_in = _roughness(pos)
    ideal = _roughness(pos + true_warps[:, [0, 3]]) / rough_in
    assert ideal < 0.1, ideal
    b, (d,) = run_context(gpu, clip)
    try:
        out, inside, warps = b.stabilize(d.ptr, w, h, weights, zoom=1.0, border=BORDER_CONSTANT, model=GM_AFFINE, rounds=3,
                                         thresh=1.0, fb_check=True, inside=True)
    finally:
        b.close()
    ratio = _roughness(pos + warps[:, [0, 3]]) / rough_in
    worst = np.abs(warps[:, [0, 3]] - true_warps[:, [0, 3]]).max()
    print(f"roughness: input {rough_in:.4f} px, stabilised / input {ratio:.4f} (with the true models: {ideal:.4f}); largest "
          f"difference between the estimated and the true warp translation {worst:.4f} px; inside on {inside.mean():.4f} of the "
          "pixels")
    assert ratio < 0.25, ratio
    assert out.shape == clip.shape and np.array_equal(out[0], clip[0]) and np.array_equal(out[-1], clip[-1])


# ------------------------------------------------------------------ 6. the command-line tool
def test_stabilize_frames_tool(gpu, tmp_path):
    """tools/stabilize_frames.py on five PNGs: <stem>_000.png ... and the CSV hold what Batch.stabilize returns for the clip"""
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
    stem = str(tmp_path / "stab")
    res = subprocess.run([sys.executable, tool, "--radius", "2", "--sigma", "1.5", "--zoom", "1.1", "--border", "replicate"]
                         + paths + [stem], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout, res.stderr)
    b, (d,) = run_context(gpu, clip)
    try:
        want = b.stabilize(d.ptr, w, h, gaussian_weights(2, 1.5), zoom=1.1, border=BORDER_REPLICATE, fb_check=True)
    finally:
        b.close()
    got = np.stack([np.asarray(Image.open(f"{stem}_{k:03d}.png")) for k in range(n + 1)])
    assert_same_bits(got, want[0], "the tool's files")
    assert (got != clip).any()
    rows = [line.split(",") for line in open(stem + ".csv").read().splitlines()]
    assert len(rows) == n + 1 and all(len(r) == 6 for r in rows)
    assert_same_bits(np.array([[float(v) for v in r] for r in rows], np.float64), want[2], "the tool's warps")
    res = subprocess.run([sys.executable, tool, "--zoom", "0.5"] + paths + [stem], capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "--zoom" in (res.stderr + res.stdout)
