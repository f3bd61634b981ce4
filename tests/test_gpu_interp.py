"""-m gpu: frame interpolation from bidirectional flow (include/ofdis.h: ofdis_interpolate on materialised arrays,
ofdis_batch_interpolate straight from a REVERSE context's level flows).

`interp_ref` restates the header's definition in numpy float32, one separately rounded operation at a time; the standalone
kernel is compared with it bit for bit, and the fused kernel bit for bit with the standalone one applied to the four outputs
of ofdis_batch_upsample_bidir."""
import math

import numpy as np
import pytest

import gen_synth
from of_dis_amd.params import oppoint, padded_size
from seq_products import FB_REJECTS, SIZE_REJECTS, assert_same_bits

pytestmark = pytest.mark.gpu
_f32 = np.float32


# ------------------------------------------------------------------ the definition, restated
def _sample(I, pxc, pyc):
    """I [h][w][noc] uint8 at the clamped points: [..., noc] float32"""
    h, w, _ = I.shape
    if w > 1:
        x0 = np.minimum(np.floor(pxc).astype(np.int64), w - 2)
        ax = pxc - x0.astype(_f32)
    else:
        x0, ax = np.zeros(pxc.shape, np.int64), np.zeros(pxc.shape, _f32)
    if h > 1:
        y0 = np.minimum(np.floor(pyc).astype(np.int64), h - 2)
        ay = pyc - y0.astype(_f32)
    else:
        y0, ay = np.zeros(pyc.shape, np.int64), np.zeros(pyc.shape, _f32)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    one = _f32(1)
    bx, by = (one - ax)[..., None], (one - ay)[..., None]
    ax, ay = ax[..., None], ay[..., None]
    If = I.astype(_f32)
    return (If[y0, x0] * bx + If[y0, x1] * ax) * by + (If[y1, x0] * bx + If[y1, x1] * ax) * ay


def interp_ref(A, B, F01, F10, M01, M10, times):
    """one frame pair: A, B [h][w][noc] uint8, F01, F10 [h][w][2] float32, masks [h][w] uint8 or None -> [nt][h][w][noc]"""
    h, w, _ = A.shape
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    xf, yf = xs.astype(_f32), ys.astype(_f32)
    u0, v0, u1, v1 = F01[..., 0], F01[..., 1], F10[..., 0], F10[..., 1]
    W1, H1 = _f32(w - 1), _f32(h - 1)
    zero, one, half = _f32(0), _f32(1), _f32(0.5)
    out = []
    with np.errstate(all="ignore"):
        for t in times:
            t = _f32(t)
            s = one - t
            a, tt, ss = s * t, t * t, s * s
            ft0x, ft0y = tt * u1 - a * u0, tt * v1 - a * v0
            ft1x, ft1y = ss * u0 - a * u1, ss * v0 - a * v1
            p0x, p0y, p1x, p1y = xf + ft0x, yf + ft0y, xf + ft1x, yf + ft1y
            clampx = lambda p: np.fmin(np.fmax(p, zero), W1)
            clampy = lambda p: np.fmin(np.fmax(p, zero), H1)
            p0xc, p0yc, p1xc, p1yc = clampx(p0x), clampy(p0y), clampx(p1x), clampy(p1y)
            c0, c1 = _sample(A, p0xc, p0yc), _sample(B, p1xc, p1yc)
            inside = lambda px, py: (px >= zero) & (px <= W1) & (py >= zero) & (py <= H1)

            def valid(M, px, py, pxc, pyc):
                v = inside(px, py)
                if M is not None:
                    nx = np.minimum(np.floor(pxc + half).astype(np.int64), w - 1)
                    ny = np.minimum(np.floor(pyc + half).astype(np.int64), h - 1)
                    v &= M[ny, nx] == 0
                return v
            va, vb = valid(M01, p0x, p0y, p0xc, p0yc), valid(M10, p1x, p1y, p1xc, p1yc)
            only_a = (one, zero) if t < one else (zero, one)
            only_b = (zero, one) if t > zero else (one, zero)
            w0 = np.where(va == vb, s, np.where(va, only_a[0], only_b[0])).astype(_f32)[..., None]
            w1 = np.where(va == vb, t, np.where(va, only_a[1], only_b[1])).astype(_f32)[..., None]
            r = np.floor((w0 * c0 + w1 * c1) + half).astype(np.int64)
            out.append(np.clip(r, 0, 255).astype(np.uint8))
    return np.stack(out)


def ref_frames(A, B, F01, F10, M01, M10, times):
    """[n] frames of interp_ref; A, B [n][h][w] or [n][h][w][3]; the result drops the channel axis for gray"""
    gray = A.ndim == 3
    if gray:
        A, B = A[..., None], B[..., None]
    out = np.stack([interp_ref(A[k], B[k], F01[k], F10[k], None if M01 is None else M01[k], None if M10 is None else M10[k],
                               times) for k in range(A.shape[0])])
    return out[..., 0] if gray else out


# ------------------------------------------------------------------ standalone kernel against the restatement
T_SETS = [
    pytest.param([0.5], id="t0.5"),
    pytest.param([0.0], id="t0"),
    pytest.param([1.0], id="t1"),
    pytest.param([0.25], id="t0.25"),
    pytest.param([float(_f32(1 / 3))], id="t1/3"),
    pytest.param([0.9999999], id="t0.9999999"),
    pytest.param([0.0, 1.0, 0.5, 0.25, float(_f32(1 / 3)), 0.9999999, 0.75], id="multi7"),
    pytest.param([i / 15 for i in range(16)], id="multi16"),
]


def _random_case(rng, n, w, h, noc, kind):
    shape = (n, h, w) + ((3,) if noc == 3 else ())
    A = rng.integers(0, 256, shape, dtype=np.uint8)
    B = rng.integers(0, 256, shape, dtype=np.uint8)
    F = [(rng.standard_normal((n, h, w, 2)) * 3).astype(_f32) for _ in range(2)]
    if kind == "wild":
        for f in F:
            pick = rng.random((n, h, w, 2))
            f[pick < 0.08] = (rng.standard_normal(int((pick < 0.08).sum())) * 1e4).astype(_f32)     # large, pointing outside
            f[(pick >= 0.08) & (pick < 0.1)] = np.inf
            f[(pick >= 0.1) & (pick < 0.12)] = -np.inf
            f[(pick >= 0.12) & (pick < 0.14)] = np.nan
            f[(pick >= 0.14) & (pick < 0.2)] = (rng.uniform(-2, 2, int(((pick >= 0.14) & (pick < 0.2)).sum())) * max(w, h)
                                                ).astype(_f32)
    M = [rng.integers(0, 3, (n, h, w), dtype=np.uint8) for _ in range(2)]
    return A, B, F[0], F[1], M[0], M[1]


SIZES = [(37, 11), (64, 16), (1, 9), (13, 1), (1, 1), (6, 5), (33, 7)]


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("kind", ["smooth", "wild"])
def test_standalone_matches_the_definition(gpu, noc, w, h, kind):
    rng = np.random.default_rng(w * 1000 + h * 10 + noc + (5 if kind == "wild" else 0))
    A, B, F01, F10, M01, M10 = _random_case(rng, 2, w, h, noc, kind)
    times = [0.0, 1.0, 0.5, 0.25, float(_f32(1 / 3)), 0.9999999]
    for masks in ((M01, M10), (None, None), (M01, None), (None, M10)):
        got = gpu.interpolate(A, B, F01, F10, times, *masks)
        want = ref_frames(A, B, F01, F10, *masks, times)
        assert_same_bits(got, want, f"noc {noc}, {w}x{h}, {kind}, masks {[m is not None for m in masks]}")


@pytest.mark.parametrize("times", T_SETS)
@pytest.mark.parametrize("noc", [1, 3])
def test_standalone_time_sets(gpu, noc, times):
    rng = np.random.default_rng(77 + noc)
    A, B, F01, F10, M01, M10 = _random_case(rng, 3, 70, 23, noc, "wild")
    assert_same_bits(gpu.interpolate(A, B, F01, F10, times, M01, M10), ref_frames(A, B, F01, F10, M01, M10, times),
                    f"noc {noc}, times {times}")


@pytest.mark.parametrize("noc", [1, 3])
def test_end_times_return_the_frames(gpu, noc):
    """finite flows: t = 0 is A and t = 1 is B bit for bit, whatever the masks"""
    rng = np.random.default_rng(5 + noc)
    A, B, F01, F10, M01, M10 = _random_case(rng, 2, 53, 19, noc, "smooth")
    F01 *= 20
    for masks in ((M01, M10), (None, None)):
        got = gpu.interpolate(A, B, F01, F10, [0.0, 1.0], *masks)
        assert_same_bits(got[:, 0], A, "t = 0")
        assert_same_bits(got[:, 1], B, "t = 1")


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", [(64, 16), (37, 11)], ids=["64x16", "37x11"])
def test_unaligned_out_takes_byte_stores_with_the_same_bytes(gpu, noc, w, h):
    """out one byte into its buffer: the same bytes as the aligned call, and the guard bytes around it stay.  64x16: rows a
    multiple of 4 pixels, so the alignment alone decides the store; 37x11: an odd width with a ragged last quad."""
    n, guard, times = 3, 257, [0.25, 0.5]   # (the array starts at byte 257 of its buffer: 1 mod 4)
    A, B, F01, F10, M01, M10 = _random_case(np.random.default_rng(900 + w + noc), n, w, h, noc, "smooth")
    want = gpu.interpolate(A, B, F01, F10, times, M01, M10)
    t = np.asarray(times, _f32)
    do = gpu.Dev(np.full(want.nbytes + 2 * guard, 0xAB, np.uint8))
    devs = [gpu.Dev(x) for x in (A, B, F01, F10, M01, M10)]
    gpu.check(gpu.lib().ofdis_interpolate(*[d.ptr for d in devs], do.ptr + guard, n, w, h, noc, t.ctypes.data_as(gpu.FP), t.size,
                                          None))
    gpu.check(gpu.lib().ofdis_sync(None))
    o = do.get((want.nbytes + 2 * guard,), np.uint8)
    assert (o[:guard] == 0xAB).all() and (o[guard + want.nbytes:] == 0xAB).all()
    assert_same_bits(o[guard:guard + want.nbytes].reshape(want.shape), want, "out, one byte off")


@pytest.mark.parametrize("d", [(4, -2), (-6, 3), (2, 0)])
def test_integer_translation(gpu, d):
    """F01 = d, F10 = -d: the output at t is A shifted by t*d wherever t*d is integral and the sample is inside"""
    w, h = 48, 20
    rng = np.random.default_rng(11)
    A = rng.integers(0, 256, (1, h, w), dtype=np.uint8)
    B = np.zeros_like(A)
    dx, dy = d
    # B(x) = A(x - d) where defined, noise elsewhere
    B[:] = rng.integers(0, 256, B.shape, dtype=np.uint8)
    ys, xs = np.mgrid[0:h, 0:w]
    src_ok = (xs - dx >= 0) & (xs - dx < w) & (ys - dy >= 0) & (ys - dy < h)
    B[0][src_ok] = A[0][(ys - dy)[src_ok], (xs - dx)[src_ok]]
    F01 = np.broadcast_to(np.array([dx, dy], _f32), (1, h, w, 2)).copy()
    F10 = -F01
    times = [0.5, 0.25, 0.75]
    got = gpu.interpolate(A, B, F01, F10, times)
    for k, t in enumerate(times):
        sx, sy = t * dx, t * dy
        if sx != int(sx) or sy != int(sy):
            continue
        sx, sy = int(sx), int(sy)
        # output pixel x samples A at x - t*d: the true frame at t is A shifted by t*d
        ok = (xs - sx >= 0) & (xs - sx < w) & (ys - sy >= 0) & (ys - sy < h)
        ok &= (xs - sx + dx >= 0) & (xs - sx + dx < w) & (ys - sy + dy >= 0) & (ys - sy + dy < h)  # B's sample inside too
        want = A[0][(ys - sy)[ok], (xs - sx)[ok]]
        assert np.array_equal(got[0, k][ok], want), (d, t)
        assert ok.sum() > 0


# ------------------------------------------------------------------ fused kernel against the standalone one
def _reverse_context(gpu, p, frames_a, frames_b, w, h, pipeline=1, contract=None):
    da, db = gpu.Dev(frames_a), gpu.Dev(frames_b)
    old = gpu.set_tuning(contract=contract) if contract is not None else None
    try:
        b = gpu.Batch(p, frames_a.shape[0], reverse=True)
        if pipeline > 1:
            b.set_pipeline(pipeline)
        b.build_pyramids_u8(da.ptr, db.ptr, w, h)
        b.run()
    finally:
        if old is not None:
            gpu.restore_tuning(old)
    return b, da, db


def _u8_frames(w, h, noc, n, seed=3100, blocks=False):
    make = gen_synth.make_pair_blocks if blocks else gen_synth.make_pair
    pairs = [make(w, h, seed + 7 * k, noc)[:2] for k in range(n)]
    return np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])


# (noc, op, w, h, n, first, count, pipeline, contract, alpha, beta)
FUSED_CASES = [
    pytest.param(1, 2, 256, 112, 3, 0, 3, 1, 0, 0.01, 0.5, id="gray-op2-scl1"),
    pytest.param(3, 2, 256, 112, 3, 0, 3, 1, 0, 0.01, 0.5, id="rgb-op2-scl1"),
    pytest.param(1, 4, 256, 112, 2, 0, 2, 1, 0, 0.01, 0.5, id="gray-op4-scl0"),
    pytest.param(3, 4, 256, 112, 2, 0, 2, 1, 0, 0.01, 0.5, id="rgb-op4-scl0"),
    pytest.param(1, 2, 250, 110, 3, 0, 3, 1, 0, 0.01, 0.5, id="gray-crop-250x110"),
    pytest.param(3, 2, 243, 107, 2, 0, 2, 1, 0, 0.01, 0.5, id="rgb-crop-243x107"),
    pytest.param(1, 2, 256, 112, 5, 1, 3, 1, 0, 0.01, 0.5, id="gray-subrange-1-3"),
    pytest.param(3, 2, 250, 110, 4, 3, 1, 1, 0, 0.01, 0.5, id="rgb-subrange-3-1"),
    pytest.param(1, 2, 256, 112, 16, 2, 13, 2, 0, 0.01, 0.5, id="gray-pipelined"),
    pytest.param(1, 2, 256, 112, 3, 0, 3, 1, 1, 0.01, 0.5, id="gray-fused-contract"),
    pytest.param(3, 2, 256, 112, 2, 0, 2, 1, 1, 0.01, 0.5, id="rgb-fused-contract"),
    pytest.param(1, 2, 256, 112, 3, 0, 3, 1, 0, 0.2, 3.0, id="gray-alpha0.2-beta3"),
    pytest.param(1, 2, 256, 112, 3, 0, 3, 1, 0, 0.0, 0.0, id="gray-alpha0-beta0"),
]


@pytest.mark.parametrize("noc,opp,w,h,n,first,count,pipeline,contract,alpha,beta", FUSED_CASES)
def test_fused_matches_standalone_on_upsample_bidir(gpu, noc, opp, w, h, n, first, count, pipeline, contract, alpha, beta):
    p = oppoint(opp, w, h, noc=noc, verbosity=0)
    p.width, p.height = padded_size(w, h, p.sc_f)
    ia, ib = _u8_frames(w, h, noc, n)
    b, da, db = _reverse_context(gpu, p, ia, ib, w, h, pipeline, contract)
    try:
        times = [0.5, 0.0, 1.0, 0.3, 0.9999999]
        fused = b.interpolate(da.ptr, db.ptr, w, h, times, first=first, count=count, alpha=alpha, beta=beta)
        fw, rev, mf, mr = b.upsample_bidir(w, h, alpha, beta, first=first, count=count)
    finally:
        b.close()
    sl = slice(first, first + count)
    standalone = gpu.interpolate(ia[sl], ib[sl], fw, rev, times, mf, mr)
    assert_same_bits(fused, standalone, "fused vs standalone on upsample_bidir's outputs")
    if count <= 2:
        assert_same_bits(standalone, ref_frames(ia[sl], ib[sl], fw, rev, mf, mr, times), "standalone vs the definition")


def test_fused_into_a_device_buffer_on_a_stream(gpu):
    """out_ptr / stream: the same bytes as the host-array form"""
    w, h = 256, 112
    p = oppoint(2, w, h, noc=1, verbosity=0)
    ia, ib = _u8_frames(w, h, 1, 2)
    b, da, db = _reverse_context(gpu, p, ia, ib, w, h)
    s = gpu.Stream()
    try:
        want = b.interpolate(da.ptr, db.ptr, w, h, [0.5, 0.75])
        out = gpu.Dev(nbytes=want.nbytes)
        assert b.interpolate(da.ptr, db.ptr, w, h, [0.5, 0.75], out_ptr=out.ptr, stream=s.ptr) is None
        gpu.check(gpu.lib().ofdis_sync(s.ptr))
        assert_same_bits(out.get(want.shape, np.uint8), want, "device-buffer form")
    finally:
        b.close()
        s.close()


# ------------------------------------------------------------------ checks that need a context
@pytest.fixture(scope="module")
def contexts(gpu):
    p = oppoint(2, 256, 112)
    plain, rev = gpu.Batch(p, 2), gpu.Batch(p, 2, reverse=True)
    yield plain, rev
    plain.close()
    rev.close()


def _batch_call(gpu, h, first=0, count=1, times=(0.5,), ntimes=None, img=True, out=True, wo=256, ho=112,
                alpha=0.01, beta=0.5, times_null=False):
    buf = np.zeros(16 * 256 * 112 * 3, np.uint8)
    t = np.asarray(times, _f32)
    return gpu.lib().ofdis_batch_interpolate(h, buf.ctypes.data if img else None, buf.ctypes.data, first, count,
                                             None if times_null else t.ctypes.data_as(gpu.FP),
                                             t.size if ntimes is None else ntimes, buf.ctypes.data if out else None, wo, ho,
                                             alpha, beta, None)


def test_batch_interpolate_rejects_a_plain_context(gpu, contexts):
    plain, _ = contexts
    assert _batch_call(gpu, plain.h) == -1
    assert "REVERSE" in gpu.lib().ofdis_last_error().decode()


@pytest.mark.parametrize("kw", [
    dict(img=False), dict(out=False), dict(times_null=True), dict(ntimes=0), dict(ntimes=17, times=[0.5] * 17),
    dict(times=[math.nan]), dict(times=[1.5]), dict(times=[-0.25]), dict(times=[math.inf]), dict(times=[0.5, -math.inf]),
    dict(first=-1), dict(count=0), dict(first=1, count=2), dict(first=2, count=1), dict(count=3),
] + SIZE_REJECTS + FB_REJECTS, ids=lambda kw: ",".join(f"{k}={v if not isinstance(v, list) else len(v)}" for k, v in kw.items()))
def test_batch_interpolate_rejects(gpu, contexts, kw):
    """host buffers stand in for the device arrays: every call returns before it would launch"""
    _, rev = contexts
    assert _batch_call(gpu, rev.h, **kw) == -1


# ------------------------------------------------------------------ quality end to end
def test_quality_against_the_true_middle_frame(gpu):
    """REVERSE context (operating point 2) on gen_synth.make_pair(256, 128, 1234), then Batch.interpolate at t = 0.5,
    against the true middle frame make_pair(..., flow_scale=0.5)[1] on the interior crop [16:-16, 16:-16].  The mean
    absolute error must be at most half that of (A + B) / 2.  Measured on an MI355X: 0.635 against 9.147, ratio 0.069."""
    w, h = 256, 128
    a, b_, _ = gen_synth.make_pair(w, h, 1234)
    mid = gen_synth.make_pair(w, h, 1234, flow_scale=0.5)[1]
    p = oppoint(2, w, h, noc=1, verbosity=0)
    p.width, p.height = padded_size(w, h, p.sc_f)
    ia, ib = a[None], b_[None]
    b, da, db = _reverse_context(gpu, p, ia, ib, w, h)
    try:
        got = b.interpolate(da.ptr, db.ptr, w, h, [0.5])[0, 0]
    finally:
        b.close()
    crop = (slice(16, -16), slice(16, -16))
    mae = np.abs(got[crop].astype(np.float64) - mid[crop]).mean()
    avg = (a.astype(np.float64) + b_) / 2
    mae_avg = np.abs(avg[crop] - mid[crop]).mean()
    print(f"interpolated MAE {mae:.3f}, (A+B)/2 MAE {mae_avg:.3f}, ratio {mae / mae_avg:.3f}")
    assert mae <= 0.5 * mae_avg, (mae, mae_avg)


@pytest.mark.parametrize("noc", [1, 3])
def test_occlusion_masks_change_the_output(gpu, noc):
    """make_pair_blocks (occlusions): the masks of upsample_bidir change some output pixels against NULL masks, and the
    fused output stays bit-equal to the definition"""
    w, h = 256, 112
    p = oppoint(2, w, h, noc=noc, verbosity=0)
    ia, ib = _u8_frames(w, h, noc, 1, seed=42, blocks=True)
    b, da, db = _reverse_context(gpu, p, ia, ib, w, h)
    try:
        times = [0.5, 0.25]
        fused = b.interpolate(da.ptr, db.ptr, w, h, times)
        fw, rev, mf, mr = b.upsample_bidir(w, h)
    finally:
        b.close()
    assert (mf != 0).any() and (mr != 0).any()
    assert_same_bits(fused, ref_frames(ia, ib, fw, rev, mf, mr, times), "fused vs the definition")
    unmasked = gpu.interpolate(ia, ib, fw, rev, times)
    assert (unmasked != fused).sum() > 0
