"""-m gpu: temporal filtering along flow trajectories over 2R + 1 frames (include/ofdis.h: ofdis_trajectory_filter on materialised
flows, ofdis_batch_trajectory_filter straight from the level flows of a SEQUENCE | REVERSE context).

The standalone kernel is compared bit for bit -- out and support -- with of_dis_amd/temporal.py: trajectory_filter_ref, the
header's definition in numpy float32, and at radius 1 with the existing ofdis_temporal_filter; the fused kernel bit for bit with
the standalone one applied to out_fw and out_rev of ofdis_batch_upsample_bidir and, for ranges of at most five frames, with the
definition as well.  Conditions on the generated inputs are checked on the restatement or the standalone result, never on the
kernel under test."""
import math

import numpy as np
import pytest

from of_dis_amd.temporal import reach, trajectory_filter_ref, trajectory_weights
from seq_products import (FB_REJECTS, FLT_MIN, INVALID, RANGE_REJECTS, SIZE_REJECTS, assert_same_bits, flag_contexts,
                          run_context, smooth_clip)
from trajfilter_cases import SIZES, coherent_case, old_support, random_case

pytestmark = pytest.mark.gpu
_f32 = np.float32


def assert_filtered_equal(got, want, what):
    assert_same_bits(got[0], want[0], what + ", out")
    assert_same_bits(got[1], want[1], what + ", support")


def _case(kind, n, w, h, noc):
    return coherent_case(n, w, h, noc) if kind == "coherent" else random_case(n, w, h, noc, kind)


# ------------------------------------------------------------------ 1. standalone kernel against the restatement
def _weights_and_tau(R):
    """flat 1 without a gate; 1, 0.5, 0.25, ... with tau 12; a zero weight in the middle; all zero; flat 1 with tau = FLT_MIN"""
    holed = np.ones(R, _f32)
    holed[R // 2] = 0.0
    return [(np.ones(R, _f32), math.inf), ((0.5 ** np.arange(R)).astype(_f32), 12.0), (holed, 24.0), (np.zeros(R, _f32), 5.0),
            (np.ones(R, _f32), FLT_MIN)]


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("kind", ["smooth", "wild", "coherent"])
def test_standalone_matches_the_definition(gpu, noc, w, h, kind):
    for npairs in (1, 3, 6):
        frames, fw, rev = _case(kind, npairs, w, h, noc)
        for R in (1, 2, 3, 8):
            for fb in (0, 1):
                for weights, tau in _weights_and_tau(R):
                    what = f"noc {noc}, {w}x{h}, {kind}, {npairs} pairs, radius {R}, fb_check {fb}, weights {weights}, tau {tau}"
                    want = trajectory_filter_ref(frames, fw, rev, weights, tau=tau, fb_check=fb)
                    got = gpu.trajectory_filter(frames, fw, rev, weights, tau=tau, fb_check=fb)
                    assert_filtered_equal(got, want, what)
                    if not weights.any():
                        assert np.array_equal(want[0], frames) and not want[1].any()
                # (conditions on the restatement) the coherent flows exercise walks of several steps under the test
                if kind == "coherent" and fb == 1 and R == 3 and npairs == 6 and w * h >= 400:
                    nb, nf = reach(trajectory_filter_ref(frames, fw, rev, np.ones(R, _f32), fb_check=1)[1])
                    full = ((nb[3] == R) & (nf[3] == R)).mean()
                    early = ((nb[3] < R) | (nf[3] < R)).mean()
                    assert full >= 0.25 and early >= 0.05, (full, early)
        # support = NULL writes the same out
        weights = trajectory_weights(2, 0.5)
        got, none = gpu.trajectory_filter(frames, fw, rev, weights, tau=12.0, support=False)
        assert none is None
        assert_same_bits(got, trajectory_filter_ref(frames, fw, rev, weights, tau=12.0)[0], "support = NULL")


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("kind", ["smooth", "wild"])
def test_radius_1_matches_the_existing_filter(gpu, noc, w, h, kind):
    """out of radius 1 is out of ofdis_temporal_filter: with masks from ofdis_fb_check for fb_check = 1, NULL masks for 0"""
    frames, fw, rev = random_case(3, w, h, noc, kind)
    for alpha, beta in ((0.01, 0.5), (0.2, 3.0)):
        mfw, mrev = gpu.fb_check(fw, rev, alpha, beta), gpu.fb_check(rev, fw, alpha, beta)
        for wn, tau in ((1.0, math.inf), (0.5, 12.0)):
            old = gpu.temporal_filter(frames, fw, rev, mfw, mrev, wn=wn, tau=tau)
            new = gpu.trajectory_filter(frames, fw, rev, [wn], tau=tau, fb_check=1, alpha=alpha, beta=beta)
            assert_filtered_equal((new[0], old_support(new[1])), old, f"fb_check 1, alpha {alpha}, wn {wn}, tau {tau}")
    for wn, tau in ((1.0, math.inf), (0.5, 12.0)):
        old = gpu.temporal_filter(frames, fw, rev, wn=wn, tau=tau)
        new = gpu.trajectory_filter(frames, fw, rev, [wn], tau=tau, fb_check=0)
        assert_filtered_equal((new[0], old_support(new[1])), old, f"fb_check 0, wn {wn}, tau {tau}")


@pytest.mark.parametrize("noc", [1, 3])
def test_identical_frames_with_zero_flows_return_the_clip(gpu, noc):
    rng = np.random.default_rng(21 + noc)
    w, h, n = 52, 9, 5
    frames = np.repeat(rng.integers(0, 256, (1, h, w) + ((3,) if noc == 3 else ()), dtype=np.uint8), n + 1, axis=0)
    z = np.zeros((n, h, w, 2), _f32)
    for R, tau in ((2, math.inf), (8, 8.0)):
        out, support = gpu.trajectory_filter(frames, z, z, trajectory_weights(R), tau=tau)
        assert_same_bits(out, frames, f"radius {R}, tau {tau}")
        nb, nf = reach(support)
        for f in range(n + 1):
            assert (nb[f] == min(R, f)).all() and (nf[f] == min(R, n - f)).all()


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", [(64, 16), (37, 11)], ids=["64x16", "37x11"])
def test_unaligned_arrays_take_byte_stores_with_the_same_bytes(gpu, noc, w, h):
    """out and support one byte into their buffers: the same bytes as the aligned call, and the guard bytes around both stay"""
    npairs, guard = 3, 257   # (the arrays start at byte 257 of their buffers: 1 mod 4)
    frames, fw, rev = coherent_case(npairs, w, h, noc)
    weights = trajectory_weights(2, 0.5)
    want = gpu.trajectory_filter(frames, fw, rev, weights, tau=12.0)
    obytes, sbytes = frames.nbytes, (npairs + 1) * h * w
    do = gpu.Dev(np.full(obytes + 2 * guard, 0xAB, np.uint8))
    ds = gpu.Dev(np.full(sbytes + 2 * guard, 0xAB, np.uint8))
    devs = [gpu.Dev(x) for x in (frames, fw, rev)]
    gpu.check(gpu.lib().ofdis_trajectory_filter(*[d.ptr for d in devs], do.ptr + guard, ds.ptr + guard, npairs, w, h, noc,
                                                weights.ctypes.data, 2, 12.0, 1, gpu.FB_ALPHA, gpu.FB_BETA, None))
    gpu.check(gpu.lib().ofdis_sync(None))
    o, s = do.get((obytes + 2 * guard,), np.uint8), ds.get((sbytes + 2 * guard,), np.uint8)
    for buf, n in ((o, obytes), (s, sbytes)):
        assert (buf[:guard] == 0xAB).all() and (buf[guard + n:] == 0xAB).all()
    assert_same_bits(o[guard:guard + obytes].reshape(frames.shape), want[0], "out, one byte off")
    assert_same_bits(s[guard:guard + sbytes].reshape(npairs + 1, h, w), want[1], "support, one byte off")
    assert (want[1] != 0).any()


def test_many_frames_map_onto_their_own_neighbours(gpu):
    """more than 8 output frames (the frame-to-XCD mapping with its padded last group) against the definition"""
    frames, fw, rev = coherent_case(10, 33, 7, 1)
    weights = trajectory_weights(3, 1.0, sigma=2.0)
    want = trajectory_filter_ref(frames, fw, rev, weights, tau=12.0)
    assert_filtered_equal(gpu.trajectory_filter(frames, fw, rev, weights, tau=12.0), want, "11 frames")
    assert (reach(want[1])[1][:8] == 3).any() and (reach(want[1])[0][3:] == 3).any()


# ------------------------------------------------------------------ 2. fused kernel against the standalone one
# (weights, tau, fb_check)
FUSED_SETTINGS = [(trajectory_weights(2), math.inf, 1), (trajectory_weights(4, 0.75, sigma=2.0), 24.0, 1),
                  (trajectory_weights(2), 24.0, 0)]

# (noc, op, w, h, n pairs, first, count, pipeline, contract, alpha, beta)
FUSED_CASES = [
    pytest.param(1, 2, 256, 112, 4, 0, 4, 1, 0, 0.01, 0.5, id="gray-op2-scl1"),
    pytest.param(3, 2, 256, 112, 4, 0, 4, 1, 0, 0.01, 0.5, id="rgb-op2-scl1"),
    pytest.param(1, 4, 256, 112, 4, 0, 4, 1, 0, 0.01, 0.5, id="gray-op4-scl0"),
    pytest.param(3, 4, 256, 112, 3, 0, 3, 1, 0, 0.01, 0.5, id="rgb-op4-scl0"),
    pytest.param(1, 2, 250, 110, 4, 0, 4, 1, 0, 0.01, 0.5, id="gray-crop-250x110"),
    pytest.param(3, 2, 250, 110, 4, 0, 4, 1, 0, 0.01, 0.5, id="rgb-crop-250x110"),
    pytest.param(1, 4, 250, 110, 3, 0, 3, 1, 0, 0.01, 0.5, id="gray-op4-crop-250x110"),
    pytest.param(1, 2, 256, 112, 6, 1, 4, 1, 0, 0.01, 0.5, id="gray-subrange-1-4-of-6"),
    pytest.param(3, 2, 250, 110, 6, 1, 4, 1, 0, 0.01, 0.5, id="rgb-subrange-1-4-of-6"),
    pytest.param(1, 2, 256, 112, 16, 0, 16, 2, 0, 0.01, 0.5, id="gray-16-pairs-pipelined"),
    pytest.param(1, 2, 256, 112, 4, 0, 4, 1, 1, 0.01, 0.5, id="gray-fused-contract"),
    pytest.param(3, 2, 256, 112, 4, 0, 4, 1, 1, 0.01, 0.5, id="rgb-fused-contract"),
    pytest.param(1, 2, 256, 112, 4, 0, 4, 1, 0, 0.2, 3.0, id="gray-alpha0.2-beta3"),
    pytest.param(1, 2, 256, 112, 4, 0, 4, 1, 0, 0.0, 0.0, id="gray-alpha0-beta0"),
]


@pytest.mark.parametrize("noc,opp,w,h,n,first,count,pipeline,contract,alpha,beta", FUSED_CASES)
def test_fused_matches_standalone_on_upsample_bidir(gpu, noc, opp, w, h, n, first, count, pipeline, contract, alpha, beta):
    clip = smooth_clip(w, h, noc, n + 1)
    b, (d,) = run_context(gpu, clip, "seq_rev", opp, contract, pipeline)
    try:
        fused = [b.trajectory_filter(d.ptr, w, h, wts, tau=tau, fb_check=fb, first=first, count=count, alpha=alpha, beta=beta,
                                     support=True) for wts, tau, fb in FUSED_SETTINGS]
        fw, rev, _, _ = b.upsample_bidir(w, h, alpha, beta, first=first, count=count, outputs=(True, True, False, False))
    finally:
        b.close()
    sub = clip[first:first + count + 1]
    for (wts, tau, fb), got in zip(FUSED_SETTINGS, fused):
        what = f"radius {len(wts)}, tau {tau}, fb_check {fb}"
        standalone = gpu.trajectory_filter(sub, fw, rev, wts, tau=tau, fb_check=fb, alpha=alpha, beta=beta)
        assert_filtered_equal(got, standalone, "fused vs standalone on upsample_bidir's outputs, " + what)
        if count + 1 <= 5:
            want = trajectory_filter_ref(sub, fw, rev, wts, tau=tau, fb_check=fb, alpha=alpha, beta=beta)
            assert_filtered_equal(standalone, want, "standalone vs the definition, " + what)
        # a walk ends at the range's first and last frame, whatever the context holds beyond them
        nb, nf = reach(got[1])
        assert not nb[0].any() and not nf[count].any()
        assert (nb[1] <= 1).all() and (nf[count - 1] <= 1).all()
        if alpha > 0.0 and count >= 4:   # the clip is gentle: interior frames do reach two steps in both directions
            assert ((nb[2:count - 1] >= 2) & (nf[2:count - 1] >= 2)).mean() > 0.25
    if alpha == 0.0 and beta == 0.0:   # (a test nothing but an exact round trip passes: most walks end at once)
        assert (reach(fused[0][1])[1][:count] == 0).mean() > 0.5


def test_fused_into_device_buffers_on_a_stream(gpu):
    """out_ptr / support pointer / stream: the same bytes as the host-array form"""
    w, h, n = 256, 112, 3
    clip = smooth_clip(w, h, 1, n + 1)
    b, (d,) = run_context(gpu, clip)
    s = gpu.Stream()
    wts = trajectory_weights(2, 0.75)
    try:
        want = b.trajectory_filter(d.ptr, w, h, wts, tau=24.0, support=True)
        only_out = b.trajectory_filter(d.ptr, w, h, wts, tau=24.0)
        out, sup = gpu.Dev(nbytes=want[0].nbytes), gpu.Dev(nbytes=want[1].nbytes)
        assert b.trajectory_filter(d.ptr, w, h, wts, tau=24.0, out_ptr=out.ptr, support=sup.ptr, stream=s.ptr) is None
        gpu.check(gpu.lib().ofdis_sync(s.ptr))
        assert_same_bits(out.get(want[0].shape, np.uint8), want[0], "device-buffer form, out")
        assert_same_bits(sup.get(want[1].shape, np.uint8), want[1], "device-buffer form, support")
        assert_same_bits(only_out, want[0], "support = NULL")
        # radius 1 on the context is the existing fused filter
        old = b.temporal_filter(d.ptr, w, h, wn=0.75, tau=24.0, support=True)
        new = b.trajectory_filter(d.ptr, w, h, [0.75], tau=24.0, support=True)
        assert_filtered_equal((new[0], old_support(new[1])), old, "radius 1 vs Batch.temporal_filter")
    finally:
        b.close()
        s.close()


# ------------------------------------------------------------------ 3. checks that need a context
@pytest.fixture(scope="module")
def contexts(gpu):
    yield from flag_contexts(gpu)


def _batch_call(gpu, b, first=0, count=3, frames=True, out=True, in_place=False, wo=256, ho=112, weights=(1.0, 0.5), radius=None,
                tau=math.inf, fb_check=1, alpha=0.01, beta=0.5):
    """host buffers stand in for the device arrays: every call returns before it would launch"""
    fr, o = np.zeros(4 * 256 * 112, np.uint8), np.zeros(4 * 256 * 112, np.uint8)
    optr = fr.ctypes.data if in_place else (o.ctypes.data if out else None)
    wts = None if weights is None else np.asarray(weights, _f32)
    return gpu.lib().ofdis_batch_trajectory_filter(b.h, fr.ctypes.data if frames else None, first, count, optr, None, wo, ho,
                                                   None if wts is None else wts.ctypes.data,
                                                   len(weights) if radius is None else radius, tau, fb_check, alpha, beta, None)


@pytest.mark.parametrize("fb_check", [0, 1])
@pytest.mark.parametrize("which,flag", [("plain", "SEQUENCE"), ("plain", "REVERSE"), ("reverse", "SEQUENCE"), ("seq", "REVERSE")])
def test_batch_form_names_the_missing_flag(gpu, contexts, which, flag, fb_check):
    assert _batch_call(gpu, contexts[which], fb_check=fb_check) == INVALID
    assert "OFDIS_BATCH_" + flag in gpu.lib().ofdis_last_error().decode()


REJECTS = [dict(frames=False), dict(out=False), dict(in_place=True), dict(weights=None, radius=2)] + RANGE_REJECTS + SIZE_REJECTS + [
    dict(radius=0), dict(radius=-1), dict(weights=(1.0,) * 9),
    dict(weights=(-0.01,)), dict(weights=(1.0, 1.01)), dict(weights=(0.5, math.nan, 0.5)), dict(weights=(math.inf,)),
    dict(tau=0.0), dict(tau=-1.0), dict(tau=math.nan), dict(tau=-math.inf), dict(tau=FLT_MIN / 2),
    dict(fb_check=2), dict(fb_check=-1)] + FB_REJECTS + [dict(fb_check=0, alpha=math.nan)]


@pytest.mark.parametrize("kw", REJECTS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_batch_form_rejects(gpu, contexts, kw):
    assert _batch_call(gpu, contexts["seq_rev"], **kw) == INVALID
    assert gpu.lib().ofdis_last_error()


# ------------------------------------------------------------------ 4. quality end to end
def test_quality_five_frames_against_three(gpu):
    """The noisy clip of test_quality_denoising_a_noisy_clip (tests/test_gpu_tfilter.py) extended to 7 frames: a clean gray clip
    of 256x128 (gen_synth's texture in smooth motion) plus independent Gaussian noise of sigma 8 per frame (seed 99), clipped to
    8 bits, operating point 2.  Batch.trajectory_filter at radius 2 (flat weights, tau inf) against Batch.temporal_filter (wn 1,
    tau inf) on frames 2..4 and the crop [16:-16, 16:-16]: the mean absolute error against the clean frames must be at most 0.89
    of the three-frame filter's -- halfway between sqrt(3 / 5) = 0.775 (five against three equally weighted frames with
    independent noise) and no gain.  Measured on an MI355X: 2.132 against 2.920 (the noisy input: 6.366), ratio 0.730, full
    reach in both directions at every pixel of the crop (below sqrt(3 / 5): a bilinear sample averages its noise over up to
    four pixels, and the centre pixel, which is not resampled, weighs 1/5 instead of 1/3)."""
    w, h, n = 256, 128, 6
    clean = smooth_clip(w, h, 1, n + 1)
    rng = np.random.default_rng(99)
    noisy = np.clip(np.rint(clean + rng.normal(0.0, 8.0, clean.shape)), 0, 255).astype(np.uint8)
    b, (d,) = run_context(gpu, noisy)
    try:
        three = b.temporal_filter(d.ptr, w, h, wn=1.0, tau=math.inf)
        five, support = b.trajectory_filter(d.ptr, w, h, trajectory_weights(2), tau=math.inf, support=True)
    finally:
        b.close()
    crop = (slice(2, 5), slice(16, -16), slice(16, -16))
    mae_in = np.abs(noisy[crop].astype(np.float64) - clean[crop]).mean()
    mae3 = np.abs(three[crop].astype(np.float64) - clean[crop]).mean()
    mae5 = np.abs(five[crop].astype(np.float64) - clean[crop]).mean()
    nb, nf = reach(support[crop])
    print(f"noisy MAE {mae_in:.3f}, three frames {mae3:.3f}, five frames {mae5:.3f}, ratio {mae5 / mae3:.3f}, "
          f"full reach at {((nb == 2) & (nf == 2)).mean():.3f} of the pixels")
    assert mae5 <= 0.89 * mae3, (mae5, mae3)


# ------------------------------------------------------------------ 5. the command-line tool
def test_temporal_filter_frames_tool_with_a_radius(gpu, tmp_path):
    """tools/temporal_filter_frames.py --radius 2 on PNGs: <stem>_000.png ... hold what Batch.trajectory_filter returns"""
    import os
    import subprocess
    import sys
    from PIL import Image
    w, h, n = 250, 107, 4
    clip = smooth_clip(w, h, 1, n + 1)
    paths = []
    for k, f in enumerate(clip):
        paths.append(str(tmp_path / f"f{k}.png"))
        Image.fromarray(f).save(paths[-1])
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "temporal_filter_frames.py")
    stem = str(tmp_path / "den")
    res = subprocess.run([sys.executable, tool, "--radius", "2", "--sigma", "1.5", "--wn", "0.75", "--tau", "24"] + paths + [stem],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout, res.stderr)
    b, (d,) = run_context(gpu, clip)
    try:
        want = b.trajectory_filter(d.ptr, w, h, trajectory_weights(2, 0.75, sigma=1.5), tau=24.0)
        three = b.temporal_filter(d.ptr, w, h, wn=0.75, tau=24.0)
    finally:
        b.close()
    got = np.stack([np.asarray(Image.open(f"{stem}_{k:03d}.png")) for k in range(n + 1)])
    assert_same_bits(got, want, "the tool's files")
    assert (got != three).any()
    res = subprocess.run([sys.executable, tool, "--radius", "9"] + paths + [stem], capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "--radius" in (res.stderr + res.stdout)
