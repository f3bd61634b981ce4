"""-m gpu: motion-compensated temporal filtering (include/ofdis.h: ofdis_temporal_filter on materialised arrays,
ofdis_batch_temporal_filter straight from the level flows of a SEQUENCE | REVERSE context).

The standalone kernel is compared bit for bit -- out and support -- with of_dis_amd/temporal.py: temporal_filter_ref, the header's
definition in numpy float32; the fused kernel bit for bit with the standalone one applied to the four outputs of
ofdis_batch_upsample_bidir and, for ranges of at most three output frames, with the definition as well.  Conditions on the
generated inputs are checked on the restatement or the standalone result, never on the kernel under test."""
import functools
import math

import numpy as np
import pytest

import gen_synth
from of_dis_amd.params import oppoint
from of_dis_amd.temporal import SUPPORT_NEXT, SUPPORT_PREV, temporal_filter_ref
from seq_products import (FB_REJECTS, FLT_MIN, INVALID, RANGE_REJECTS, SIZE_REJECTS, assert_same_bits, flag_contexts,
                          run_context, smooth_clip)

pytestmark = pytest.mark.gpu
_f32 = np.float32


def assert_filtered_equal(got, want, what):
    assert_same_bits(got[0], want[0], what + ", out")
    assert_same_bits(got[1], want[1], what + ", support")


# ------------------------------------------------------------------ 1. standalone kernel against the restatement
SIZES = [(37, 11), (64, 16), (1, 9), (13, 1), (1, 1), (6, 5), (33, 7)]
WN_TAU = [(1.0, math.inf), (0.5, 12.0), (1.0, 1.5), (0.0, 5.0), (1.0, FLT_MIN)]


@functools.lru_cache(maxsize=None)
def _random_case(n, w, h, noc, kind):
    """npairs = n.  Flows as _random_case of tests/test_gpu_interp.py makes them: "smooth" = normal flows of 3 px, "wild" = the
    same with large, infinite, NaN and image-sized values mixed in; masks with all three codes.  Frames: "wild" uniform random
    bytes; "smooth" a ramp plus noise of a few grey levels, so that the finite gates tau = 12 and 1.5 leave weights strictly
    between 0 and wn."""
    rng = np.random.default_rng(w * 1000 + h * 10 + noc + 100 * n + (5 if kind == "wild" else 0))
    shape = (n + 1, h, w) + ((3,) if noc == 3 else ())
    if kind == "wild":
        frames = rng.integers(0, 256, shape, dtype=np.uint8)
    else:
        ys, xs = np.mgrid[0:h, 0:w]
        ramp = (40 + 1.5 * xs + 2.5 * ys).reshape((1, h, w) + ((1,) if noc == 3 else ()))
        frames = np.clip(np.rint(ramp + rng.normal(0, 2.0, shape)), 0, 255).astype(np.uint8)
    F = [(rng.standard_normal((n, h, w, 2)) * 3).astype(_f32) for _ in range(2)]
    if kind == "wild":
        for f in F:
            pick = rng.random((n, h, w, 2))
            f[pick < 0.08] = (rng.standard_normal(int((pick < 0.08).sum())) * 1e4).astype(_f32)
            f[(pick >= 0.08) & (pick < 0.1)] = np.inf
            f[(pick >= 0.1) & (pick < 0.12)] = -np.inf
            f[(pick >= 0.12) & (pick < 0.14)] = np.nan
            sized = (pick >= 0.14) & (pick < 0.2)
            f[sized] = (rng.uniform(-2, 2, int(sized.sum())) * max(w, h)).astype(_f32)
    else:
        for f in F:
            f[rng.random((n, h, w)) < 0.3] = 0.0   # also pixels that stay put
    M = [rng.integers(0, 3, (n, h, w), dtype=np.uint8) for _ in range(2)]
    return frames, F[0], F[1], M[0], M[1]


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("kind", ["smooth", "wild"])
def test_standalone_matches_the_definition(gpu, noc, w, h, kind):
    partial = 0
    for npairs in (1, 3):
        frames, fw, rev, mfw, mrev = _random_case(npairs, w, h, noc, kind)
        for masks in ((mfw, mrev), (None, None), (mfw, None), (None, mrev)):
            for wn, tau in WN_TAU:
                what = f"noc {noc}, {w}x{h}, {kind}, {npairs} pairs, masks {[m is not None for m in masks]}, wn {wn}, tau {tau}"
                want = temporal_filter_ref(frames, fw, rev, *masks, wn=wn, tau=tau)
                assert_filtered_equal(gpu.temporal_filter(frames, fw, rev, *masks, wn=wn, tau=tau), want, what)
                if wn == 0.0:
                    assert np.array_equal(want[0], frames) and not want[1].any()
                if masks[0] is None and masks[1] is None and tau == 12.0:
                    partial += int((want[1] != 0).sum())
        # support = NULL writes the same out
        got, none = gpu.temporal_filter(frames, fw, rev, mfw, mrev, wn=0.5, tau=12.0, support=False)
        assert none is None
        assert_same_bits(got, temporal_filter_ref(frames, fw, rev, mfw, mrev, wn=0.5, tau=12.0)[0], "support = NULL")
    if kind == "smooth" and w * h >= 200:   # the finite gate is exercised with weights > 0 (condition on the restatement)
        assert partial > 0


@pytest.mark.parametrize("noc", [1, 3])
def test_identical_frames_with_zero_flows_return_the_clip(gpu, noc):
    rng = np.random.default_rng(21 + noc)
    w, h, n = 52, 9, 3
    frames = np.repeat(rng.integers(0, 256, (1, h, w) + ((3,) if noc == 3 else ()), dtype=np.uint8), n + 1, axis=0)
    z = np.zeros((n, h, w, 2), _f32)
    for tau in (math.inf, 8.0):
        out, support = gpu.temporal_filter(frames, z, z, wn=1.0, tau=tau)
        assert_same_bits(out, frames, f"tau {tau}")
        assert (support[0] == SUPPORT_NEXT).all() and (support[n] == SUPPORT_PREV).all() and (support[1:n] == 3).all()


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", [(64, 16), (37, 11)], ids=["64x16", "37x11"])
def test_unaligned_arrays_take_byte_stores_with_the_same_bytes(gpu, noc, w, h):
    """out and support one byte into their buffers: the same bytes as the aligned call, and the guard bytes around both stay"""
    npairs, guard = 3, 257   # (the arrays start at byte 257 of their buffers: 1 mod 4)
    frames, fw, rev, mfw, mrev = _random_case(npairs, w, h, noc, "smooth")
    want = gpu.temporal_filter(frames, fw, rev, mfw, mrev, wn=0.5, tau=12.0)
    obytes, sbytes = frames.nbytes, (npairs + 1) * h * w
    do = gpu.Dev(np.full(obytes + 2 * guard, 0xAB, np.uint8))
    ds = gpu.Dev(np.full(sbytes + 2 * guard, 0xAB, np.uint8))
    devs = [gpu.Dev(x) for x in (frames, fw, rev, mfw, mrev)]
    gpu.check(gpu.lib().ofdis_temporal_filter(*[d.ptr for d in devs], do.ptr + guard, ds.ptr + guard, npairs, w, h, noc, 0.5,
                                              12.0, None))
    gpu.check(gpu.lib().ofdis_sync(None))
    o, s = do.get((obytes + 2 * guard,), np.uint8), ds.get((sbytes + 2 * guard,), np.uint8)
    for buf, n in ((o, obytes), (s, sbytes)):
        assert (buf[:guard] == 0xAB).all() and (buf[guard + n:] == 0xAB).all()
    assert_same_bits(o[guard:guard + obytes].reshape(frames.shape), want[0], "out, one byte off")
    assert_same_bits(s[guard:guard + sbytes].reshape(npairs + 1, h, w), want[1], "support, one byte off")


def test_many_frames_map_onto_their_own_neighbours(gpu):
    """more than 8 output frames (the frame-to-XCD mapping with its padded last group) against the definition"""
    frames, fw, rev, mfw, mrev = _random_case(10, 33, 7, 1, "smooth")
    want = temporal_filter_ref(frames, fw, rev, mfw, mrev, wn=1.0, tau=12.0)
    assert_filtered_equal(gpu.temporal_filter(frames, fw, rev, mfw, mrev, wn=1.0, tau=12.0), want, "11 frames")


# ------------------------------------------------------------------ 2. fused kernel against the standalone one
FUSED_WN_TAU = [(1.0, math.inf), (0.75, 24.0)]

# (noc, op, w, h, n pairs, first, count, pipeline, contract, alpha, beta)
FUSED_CASES = [
    pytest.param(1, 2, 256, 112, 3, 0, 3, 1, 0, 0.01, 0.5, id="gray-op2-scl1"),
    pytest.param(3, 2, 256, 112, 3, 0, 3, 1, 0, 0.01, 0.5, id="rgb-op2-scl1"),
    pytest.param(1, 4, 256, 112, 2, 0, 2, 1, 0, 0.01, 0.5, id="gray-op4-scl0"),
    pytest.param(3, 4, 256, 112, 2, 0, 2, 1, 0, 0.01, 0.5, id="rgb-op4-scl0"),
    pytest.param(1, 2, 250, 110, 3, 0, 3, 1, 0, 0.01, 0.5, id="gray-crop-250x110"),
    pytest.param(3, 2, 243, 107, 2, 0, 2, 1, 0, 0.01, 0.5, id="rgb-crop-243x107"),
    pytest.param(1, 2, 256, 112, 5, 1, 3, 1, 0, 0.01, 0.5, id="gray-subrange-1-3-of-5"),
    pytest.param(3, 2, 250, 110, 4, 3, 1, 1, 0, 0.01, 0.5, id="rgb-subrange-3-1-of-4"),
    pytest.param(1, 2, 256, 112, 16, 0, 16, 2, 0, 0.01, 0.5, id="gray-16-pairs-pipelined"),
    pytest.param(1, 2, 256, 112, 3, 0, 3, 1, 1, 0.01, 0.5, id="gray-fused-contract"),
    pytest.param(3, 2, 256, 112, 2, 0, 2, 1, 1, 0.01, 0.5, id="rgb-fused-contract"),
    pytest.param(1, 2, 256, 112, 3, 0, 3, 1, 0, 0.2, 3.0, id="gray-alpha0.2-beta3"),
    pytest.param(1, 2, 256, 112, 3, 0, 3, 1, 0, 0.0, 0.0, id="gray-alpha0-beta0"),
]


@pytest.mark.parametrize("noc,opp,w,h,n,first,count,pipeline,contract,alpha,beta", FUSED_CASES)
def test_fused_matches_standalone_on_upsample_bidir(gpu, noc, opp, w, h, n, first, count, pipeline, contract, alpha, beta):
    clip = smooth_clip(w, h, noc, n + 1)
    b, (d,) = run_context(gpu, clip, "seq_rev", opp, contract, pipeline)
    try:
        fused = [b.temporal_filter(d.ptr, w, h, wn=wn, tau=tau, first=first, count=count, alpha=alpha, beta=beta, support=True)
                 for wn, tau in FUSED_WN_TAU]
        fw, rev, mf, mr = b.upsample_bidir(w, h, alpha, beta, first=first, count=count)
    finally:
        b.close()
    sub = clip[first:first + count + 1]
    for (wn, tau), got in zip(FUSED_WN_TAU, fused):
        standalone = gpu.temporal_filter(sub, fw, rev, mf, mr, wn=wn, tau=tau)
        assert_filtered_equal(got, standalone, f"fused vs standalone on upsample_bidir's outputs, wn {wn}, tau {tau}")
        if count + 1 <= 3:
            assert_filtered_equal(standalone, temporal_filter_ref(sub, fw, rev, mf, mr, wn=wn, tau=tau),
                                  f"standalone vs the definition, wn {wn}, tau {tau}")
        # the range's end frames use ONE neighbour, whatever the context holds beyond them
        support = got[1]
        assert (support[0] & SUPPORT_PREV == 0).all() and (support[count] & SUPPORT_NEXT == 0).all()
        if alpha > 0.0:   # the clip is gentle: neighbours do enter the averages that were compared
            assert (support[0] & SUPPORT_NEXT).any() and (support[count] & SUPPORT_PREV).any()
            assert count == 1 or (support[1:count] == 3).mean() > 0.25
    if alpha == 0.0 and beta == 0.0:   # (a test nothing but an exact round trip passes: the masks matter here)
        assert (mf != 0).mean() > 0.5


def test_fused_into_device_buffers_on_a_stream(gpu):
    """out_ptr / support pointer / stream: the same bytes as the host-array form"""
    w, h, n = 256, 112, 2
    clip = smooth_clip(w, h, 1, n + 1)
    b, (d,) = run_context(gpu, clip)
    s = gpu.Stream()
    try:
        want = b.temporal_filter(d.ptr, w, h, wn=0.75, tau=24.0, support=True)
        only_out = b.temporal_filter(d.ptr, w, h, wn=0.75, tau=24.0)
        out, sup = gpu.Dev(nbytes=want[0].nbytes), gpu.Dev(nbytes=want[1].nbytes)
        assert b.temporal_filter(d.ptr, w, h, wn=0.75, tau=24.0, out_ptr=out.ptr, support=sup.ptr, stream=s.ptr) is None
        gpu.check(gpu.lib().ofdis_sync(s.ptr))
        assert_same_bits(out.get(want[0].shape, np.uint8), want[0], "device-buffer form, out")
        assert_same_bits(sup.get(want[1].shape, np.uint8), want[1], "device-buffer form, support")
        assert_same_bits(only_out, want[0], "support = NULL")
    finally:
        b.close()
        s.close()


@pytest.mark.parametrize("noc", [1, 3])
def test_occlusion_masks_change_the_output(gpu, noc):
    """gen_synth.make_pair_blocks (occlusions) as the clip a, b, a, b: in the interior frames some pixels lose a neighbour, the
    fused output is the definition's, and it differs from the standalone result with NULL masks"""
    w, h = 256, 112
    a, b_ = gen_synth.make_pair_blocks(w, h, 42, noc)
    clip = np.ascontiguousarray(np.stack([a, b_, a, b_]))
    b, (d,) = run_context(gpu, clip)
    try:
        fused = b.temporal_filter(d.ptr, w, h, support=True)
        fw, rev, mf, mr = b.upsample_bidir(w, h)
    finally:
        b.close()
    assert (mf != 0).any() and (mr != 0).any()
    want = temporal_filter_ref(clip[:3], fw[:2], rev[:2], mf[:2], mr[:2])   # frames 0 and 1 do not depend on pair 2
    assert_same_bits(fused[0][:2], want[0][:2], "fused vs the definition, out")
    assert_same_bits(fused[1][:2], want[1][:2], "fused vs the definition, support")
    assert_filtered_equal(fused, gpu.temporal_filter(clip, fw, rev, mf, mr), "fused vs standalone")
    assert (fused[1][1:3] != 3).any()
    unmasked = gpu.temporal_filter(clip, fw, rev)
    assert (unmasked[0] != fused[0]).sum() > 0


# ------------------------------------------------------------------ 3. checks that need a context
@pytest.fixture(scope="module")
def contexts(gpu):
    yield from flag_contexts(gpu)


def _batch_call(gpu, b, first=0, count=3, frames=True, out=True, in_place=False, wo=256, ho=112, wn=1.0, tau=math.inf,
                alpha=0.01, beta=0.5):
    """host buffers stand in for the device arrays: every call returns before it would launch"""
    fr, o = np.zeros(4 * 256 * 112, np.uint8), np.zeros(4 * 256 * 112, np.uint8)
    optr = fr.ctypes.data if in_place else (o.ctypes.data if out else None)
    return gpu.lib().ofdis_batch_temporal_filter(b.h, fr.ctypes.data if frames else None, first, count, optr, None, wo, ho, wn,
                                                 tau, alpha, beta, None)


@pytest.mark.parametrize("which,flag", [("plain", "SEQUENCE"), ("plain", "REVERSE"), ("reverse", "SEQUENCE"), ("seq", "REVERSE")])
def test_batch_temporal_filter_names_the_missing_flag(gpu, contexts, which, flag):
    assert _batch_call(gpu, contexts[which]) == INVALID
    assert "OFDIS_BATCH_" + flag in gpu.lib().ofdis_last_error().decode()


REJECTS = [dict(frames=False), dict(out=False), dict(in_place=True)] + RANGE_REJECTS + SIZE_REJECTS + [
    dict(wn=-0.01), dict(wn=1.01), dict(wn=math.nan), dict(wn=math.inf),
    dict(tau=0.0), dict(tau=-1.0), dict(tau=math.nan), dict(tau=-math.inf), dict(tau=FLT_MIN / 2)] + FB_REJECTS


@pytest.mark.parametrize("kw", REJECTS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_batch_temporal_filter_rejects(gpu, contexts, kw):
    assert _batch_call(gpu, contexts["seq_rev"], **kw) == INVALID
    assert gpu.lib().ofdis_last_error()


def test_batch_temporal_filter_rejects_noc_2(gpu):
    """noc comes from the context's parameters, which ofdis_batch_create already holds to 1 or 3"""
    p = oppoint(2, 256, 112)
    p.noc = 2
    with pytest.raises(gpu.OfdisError):
        gpu.Batch(p, 3, sequence=True, reverse=True)


# ------------------------------------------------------------------ 4. quality end to end
def test_quality_denoising_a_noisy_clip(gpu):
    """A clean 5-frame gray clip of 256x128 (gen_synth's texture in smooth motion) plus independent Gaussian noise of sigma 8
    per frame (seed 99), clipped to 8 bits; Batch.temporal_filter(wn=1, tau=inf) at operating point 2 on the noisy clip.  The
    mean absolute error of the three interior output frames against the clean frames on the crop [16:-16, 16:-16], over the
    same error of the noisy input frames, must be at most (1 + 0.58) / 2 = 0.79: halfway between three equally weighted
    frames with independent noise (1 / sqrt(3) = 0.58) and no effect.  The slack is for pixels the consistency test drops and
    for the flow's own error on noisy frames.  Measured on an MI355X: 2.921 against 6.376, ratio 0.458, both neighbours at every
    pixel of the crop (below 1 / sqrt(3): a neighbour's bilinear sample averages its noise over up to four pixels as well)."""
    w, h, n = 256, 128, 4
    clean = smooth_clip(w, h, 1, n + 1)
    rng = np.random.default_rng(99)
    noisy = np.clip(np.rint(clean + rng.normal(0.0, 8.0, clean.shape)), 0, 255).astype(np.uint8)
    b, (d,) = run_context(gpu, noisy)
    try:
        out, support = b.temporal_filter(d.ptr, w, h, wn=1.0, tau=math.inf, support=True)
    finally:
        b.close()
    crop = (slice(1, n), slice(16, -16), slice(16, -16))
    mae_in = np.abs(noisy[crop].astype(np.float64) - clean[crop]).mean()
    mae_out = np.abs(out[crop].astype(np.float64) - clean[crop]).mean()
    print(f"noisy MAE {mae_in:.3f}, filtered MAE {mae_out:.3f}, ratio {mae_out / mae_in:.3f}, "
          f"both neighbours at {(support[crop] == 3).mean():.3f} of the pixels")
    assert mae_out <= 0.79 * mae_in, (mae_out, mae_in)


# ------------------------------------------------------------------ 5. the command-line tool
def test_temporal_filter_frames_tool(gpu, tmp_path):
    """tools/temporal_filter_frames.py on PNGs: <stem>_000.png ... hold what Batch.temporal_filter returns for the same clip"""
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
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "temporal_filter_frames.py")
    stem = str(tmp_path / "den")
    res = subprocess.run([sys.executable, tool, "--wn", "0.75", "--tau", "24"] + paths + [stem], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, (res.stdout, res.stderr)
    b, (d,) = run_context(gpu, clip)
    try:
        want = b.temporal_filter(d.ptr, w, h, wn=0.75, tau=24.0)
    finally:
        b.close()
    got = np.stack([np.asarray(Image.open(f"{stem}_{k:03d}.png")) for k in range(n + 1)])
    assert_same_bits(got, want, "the tool's files")
    assert (got != clip).any()
    res = subprocess.run([sys.executable, tool, "--wn", "1.5"] + paths + [stem], capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "--wn" in (res.stderr + res.stdout)
