"""-m gpu: the output encodings (include/ofdis.h: ofdis_encoding).  ofdis_encode against the numpy model of the header's
arithmetic (of_dis_amd/encoding.py), and ofdis_batch_upsample_frames_enc against the materialised composition
ofdis_encode(ofdis_batch_upsample_frames(...)).  Every comparison is bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

from common import synth_case
from of_dis_amd import encoding
from of_dis_amd.params import oppoint

pytestmark = pytest.mark.gpu
_f32 = np.float32

ENCODINGS = {
    "f32": encoding.F32,
    "f16": encoding.F16,
    "kitti": encoding.KITTI_FLOW,
    "disparity": encoding.KITTI_DISPARITY,
    "u8": encoding.u8_bound(20),
    "u16-fine": encoding.Encoding(2, 1000.0, 1234.5),   # spreads the test flows over much of the 16-bit range
    "u8-fine": encoding.Encoding(3, -17.25, 100.0),
}


def _same_bits(a, b, what):
    """equal element for element as bit patterns (so -0 != +0 and NaN payloads count), with a readable first difference"""
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    ua, ub = (x.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[x.dtype.itemsize]) for x in (a, b))
    if not np.array_equal(ua, ub):
        bad = np.argwhere(ua != ub)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {a.size} elements differ; first at {i}: {a[i]!r} vs {b[i]!r}")


# ------------------------------------------------------------------ ofdis_encode against the numpy model
def _crafted():
    """values that sit on every edge of the four encodings"""
    half_sub = [2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 6e-8, 2.98e-8,
                1e-7, 3.1e-5, 5.9e-8, 6.09e-5, 1e-10]                      # the subnormal range of binary16 and just below it
    half_top = [65504.0, 65519.0, 65519.996, 65520.0, 65536.0, 1e5, 3e38]   # half overflow
    half_ties = [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2048.5, 2049.5, 0.1, 1 / 3]
    k = [i / 128 for i in range(-5, 6)] + [511.984375, 512.0, 511.99, -512.0, -511.9921875, -512.01, 600.0]  # KITTI flow edges
    d = [-i / 512 for i in range(0, 8)] + [-255.998046875, -256.0, -255.99, 0.001]                             # disparity edges
    b = [0.0, 20.0, -20.0, 19.99, -19.99, 20.01, 4.0, -4.0, 0.07843137, 2 / 51, 25.0, -25.0]                   # bound-20 edges
    plain = [0.5, 1.5, 2.5, 254.5, 255.5, 65534.5, 65535.5, 0.49999997, 254.49998, -0.5, 1e9, -1e9]
    v = half_sub + half_top + half_ties + k + d + b + plain
    v = np.array(v + [-x for x in v] + [0.0, -0.0, math.inf, -math.inf], _f32)
    return v


@pytest.mark.parametrize("name", sorted(ENCODINGS))
def test_encode_crafted_values(gpu, name):
    enc = ENCODINGS[name]
    v = _crafted()
    got, want = gpu.encode(v, enc), encoding.encode(v, enc)
    print(name, "crafted:", v.size, "values,", int((got.view(np.uint8) != want.view(np.uint8)).sum()), "bytes differ")
    _same_bits(got, want, f"ofdis_encode {name} vs the numpy model")
    if name == "f16":  # the conversion must not flush: subnormal halves are among the results
        sub = (got.view(np.uint16) & 0x7c00 == 0) & (got.view(np.uint16) & 0x03ff != 0)
        assert sub.sum() >= 10, got[sub]


@pytest.mark.parametrize("name", sorted(ENCODINGS))
def test_encode_nan(gpu, name):
    enc = ENCODINGS[name]
    v = np.array([math.nan, 1.0, -math.nan, 2.0] * 5, _f32)
    got = gpu.encode(v, enc)
    if enc.type in (gpu.ENC_F32, gpu.ENC_F16):
        assert np.isnan(got[0::2]).all() and not np.isnan(got[1::2]).any()
    else:
        assert (got[0::2] == 0).all()
        _same_bits(got, encoding.encode(v, enc), name)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 64, 1000003])
@pytest.mark.parametrize("name", ["f32", "f16", "kitti", "u8"])
def test_encode_lengths(gpu, name, n):
    """whole 16-byte stores, the scalar tail, and lengths below one store"""
    enc = ENCODINGS[name]
    rng = np.random.default_rng(n)
    v = (rng.standard_normal(n) * 12).astype(_f32)
    v[rng.integers(0, n, max(1, n // 50))] *= 1e-6  # some values in half's subnormal range
    # guard elements behind the destination: written by nothing
    es = enc.dtype.itemsize
    ds, dd = gpu.Dev(v), gpu.Dev(np.full(n * es + 64, 0xA5, np.uint8))
    gpu.check(gpu.lib().ofdis_encode(ds.ptr, dd.ptr, n, C.byref(enc), None))
    gpu.check(gpu.lib().ofdis_sync(None))
    raw = dd.get((n * es + 64,), np.uint8)
    _same_bits(raw[:n * es].view(enc.dtype), encoding.encode(v, enc), f"{name}, n = {n}")
    assert (raw[n * es:] == 0xA5).all(), "ofdis_encode wrote behind its destination"


def test_encode_unaligned_arrays(gpu):
    """src or dst off the 16-byte grid: the element-wise path, same bits"""
    v = (np.random.default_rng(3).standard_normal(1000) * 30).astype(_f32)
    for name in ("f16", "kitti", "u8", "f32"):
        enc = ENCODINGS[name]
        es = enc.dtype.itemsize
        for so, do in ((1, 0), (0, 1), (3, 2)):
            ds = gpu.Dev(np.concatenate([np.zeros(so, _f32), v]))
            dd = gpu.Dev(np.full(1000 * es + 64, 0x5A, np.uint8))
            gpu.check(gpu.lib().ofdis_encode(ds.ptr + 4 * so, dd.ptr + do * 4, 1000, C.byref(enc), None))
            gpu.check(gpu.lib().ofdis_sync(None))
            raw = dd.get((1000 * es + 64,), np.uint8)
            _same_bits(raw[4 * do:4 * do + 1000 * es].view(enc.dtype), encoding.encode(v, enc), f"{name} offsets {so}, {do}")
            assert (raw[:4 * do] == 0x5A).all() and (raw[4 * do + 1000 * es:] == 0x5A).all()


# ------------------------------------------------------------------ fused == materialised composition
def _frames(w, h, noc, seeds):
    pairs = [synth_case(w, h, s, noc)[4] for s in seeds]
    return np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])


def _context(gpu, w, h, noc=1, opp=2, sc_l=None, stereo=False, n=3, seed=7300, pipeline=0, **kw):
    p = oppoint(opp, w, h, noc=noc)
    if sc_l is not None:
        p = p.copy(sc_l=sc_l)
    if stereo:
        p = p.copy(selectmode=2)
    ia, ib = _frames(w, h, noc, [seed + k for k in range(n)])
    b = gpu.Batch(p, n, **kw)
    if pipeline:
        b.set_pipeline(pipeline)
    da, db = gpu.Dev(ia), gpu.Dev(ib)
    b.build_pyramids_u8(da.ptr, db.ptr, w, h)
    b.run()
    if not pipeline:
        gpu.check(gpu.lib().ofdis_sync(None))
    return b, p, (da, db)


def _fused_with_guards(gpu, b, first, count, w, h, enc, offset=0):
    """ofdis_batch_upsample_frames_enc into the middle of a poisoned buffer: (result, guards untouched).  offset: bytes the
    output starts off the 256-byte grid of the allocation (the narrower-store paths)."""
    shape = (count, h, w, b.p.nop)
    nbytes = int(np.prod(shape)) * enc.dtype.itemsize
    G = 4096
    d = gpu.Dev(np.full(nbytes + 2 * G, 0xC3, np.uint8))
    gpu.check(gpu.lib().ofdis_batch_upsample_frames_enc(b.h, first, count, d.ptr + G + offset, w, h, C.byref(enc), None))
    gpu.check(gpu.lib().ofdis_sync(None))
    raw = d.get((nbytes + 2 * G,), np.uint8)
    ok = bool((raw[:G + offset] == 0xC3).all() and (raw[G + offset + nbytes:] == 0xC3).all())
    return raw[G + offset:G + offset + nbytes].copy().view(enc.dtype).reshape(shape), ok


def _check_context(gpu, b, w, h, first, count, what, names=None, offsets=(0,)):
    ref = b.upsample_frames(first, count, w, h)
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0.25, "a flow worth encoding"
    for name in names or sorted(ENCODINGS):
        enc = ENCODINGS[name]
        want = gpu.encode(ref, enc)
        _same_bits(want, encoding.encode(ref, enc), f"{what}: ofdis_encode {name} vs the numpy model")
        _same_bits(b.upsample_frames_enc(first, count, w, h, enc), want, f"{what}: fused {name} vs the composition")
        for off in offsets:
            if off % enc.dtype.itemsize:  # (`out` is aligned to its element)
                continue
            got, guards = _fused_with_guards(gpu, b, first, count, w, h, enc, off)
            _same_bits(got, want, f"{what}: fused {name} (guarded, offset {off}) vs the composition")
            assert guards, f"{what}: {name} wrote outside `out` (offset {off})"


CASES = [
    # w, h, noc, opp, sc_l, stereo, n, first, count
    (256, 112, 1, 2, 1, False, 3, 0, 3),      # gray, x 2, no crop, rows of 16-byte multiples for every encoding
    (256, 112, 1, 2, 2, False, 3, 1, 1),      # x 4, a frame in the middle of the batch
    (321, 239, 1, 3, 0, False, 3, 1, 2),      # x 1, odd width and height: crop on every side, narrow stores
    (333, 251, 1, 2, 1, False, 4, 1, 2),      # odd width, x 2, asymmetric crop, sub-range in the middle
    (250, 110, 3, 2, 1, False, 3, 1, 2),      # RGB, even width that is no multiple of 8, crop
    (250, 110, 3, 2, 2, False, 2, 0, 2),      # RGB, x 4
    (256, 112, 1, 2, 1, True, 3, 0, 3),       # stereo depth: one channel
    (333, 251, 1, 2, 2, True, 3, 1, 1),       # stereo, odd width, x 4, crop
    (321, 239, 1, 3, 0, True, 2, 0, 2),       # stereo, x 1
    (1024, 436, 1, 2, None, False, 2, 0, 2),  # the measured geometry (x 8, vertical crop)
]


@pytest.mark.parametrize("contract", [0, 1], ids=["exact", "fused"])
@pytest.mark.parametrize("w,h,noc,opp,sc_l,stereo,n,first,count", CASES)
def test_fused_equals_composition(gpu, contract, w, h, noc, opp, sc_l, stereo, n, first, count):
    old = gpu.set_tuning(contract=contract)
    try:
        b, p, keep = _context(gpu, w, h, noc, opp, sc_l, stereo, n)
        assert b.p.nop == (1 if stereo else 2)
        what = f"{w}x{h} noc {noc} sc_l {p.sc_l} {'stereo' if stereo else 'flow'} contract {contract} frames {first}+{count}"
        # offsets: 16-byte aligned, then 8 / 4 / 2 / 1-byte aligned outputs (every narrower-store path)
        _check_context(gpu, b, w, h, first, count, what, offsets=(0, 8, 4, 2, 1) if contract == 0 else (0,))
        b.close()
    finally:
        gpu.restore_tuning(old)


@pytest.mark.parametrize("contract", [0, 1], ids=["exact", "fused"])
def test_fused_on_a_pipelined_context(gpu, contract):
    """the call joins the pass by itself: no ofdis_batch_join, no synchronisation between run and the encoded upsample"""
    old = gpu.set_tuning(contract=contract)
    try:
        w, h = 256, 112
        plain, p, keep0 = _context(gpu, w, h, n=8)
        ref = plain.upsample_frames(2, 5, w, h)
        for sub in (2, 4):
            b, _, keep = _context(gpu, w, h, n=8, pipeline=sub)
            for name in sorted(ENCODINGS):
                enc = ENCODINGS[name]
                b.run()  # a fresh pass in flight on the internal streams
                _same_bits(b.upsample_frames_enc(2, 5, w, h, enc), gpu.encode(ref, enc), f"pipelined x{sub} {name}")
            b.close()
        plain.close()
    finally:
        gpu.restore_tuning(old)


@pytest.mark.parametrize("contract", [0, 1], ids=["exact", "fused"])
def test_fused_on_a_reverse_context(gpu, contract):
    """OFDIS_BATCH_REVERSE: the forward result"""
    old = gpu.set_tuning(contract=contract)
    try:
        w, h = 333, 251
        b, p, keep = _context(gpu, w, h, n=3, reverse=True)
        plain, _, keep2 = _context(gpu, w, h, n=3)
        _same_bits(b.upsample_frames(1, 2, w, h), plain.upsample_frames(1, 2, w, h), "forward flow of the reverse context")
        _check_context(gpu, b, w, h, 1, 2, f"reverse context, contract {contract}")
        b.close()
        plain.close()
    finally:
        gpu.restore_tuning(old)


def test_fused_on_a_stereo_lr_context(gpu):
    """OFDIS_BATCH_STEREO_LR: the forward (left-view) result"""
    w, h = 256, 112
    b, p, keep = _context(gpu, w, h, stereo=True, n=2, stereo_lr=True)
    _check_context(gpu, b, w, h, 0, 2, "stereo_lr context", names=["f32", "f16", "disparity", "u8"])
    b.close()


# ------------------------------------------------------------------ argument errors of the context call
def test_context_errors(gpu):
    L = gpu.lib()
    w, h = 256, 112
    b, p, keep = _context(gpu, w, h, n=2)
    d = gpu.Dev(nbytes=2 * w * h * 2 * 4)
    call = lambda first, count, wo, ho, enc, out=d.ptr, ctx=b.h: L.ofdis_batch_upsample_frames_enc(
        ctx, first, count, out, wo, ho, C.byref(enc) if enc is not None else None, None)
    f16 = encoding.F16
    assert call(0, 2, w, h, f16) == 0
    for first, count in ((0, 3), (2, 1), (-1, 1), (0, 0), (1, 2), (0, -1)):  # a frame range outside the batch
        assert call(first, count, w, h, f16) == -1, (first, count)
        assert L.ofdis_last_error()
    for wo, ho in ((p.width + 1, h), (w, p.height + 1), (0, h), (w, 0)):        # an original size above the padded size
        assert call(0, 2, wo, ho, f16) == -1, (wo, ho)
    assert call(0, 2, w, h, f16, out=None) == -1
    assert call(0, 2, w, h, f16, ctx=None) == -1
    assert call(0, 2, w, h, None) == -1
    bad = [gpu.Encoding(t, 1.0, 0.0) for t in (-1, 4, 99)]
    bad += [gpu.Encoding(t, s, 0.0) for t in (gpu.ENC_U16, gpu.ENC_U8) for s in (0.0, math.inf, -math.inf, math.nan)]
    bad += [gpu.Encoding(t, 1.0, o) for t in (gpu.ENC_U16, gpu.ENC_U8) for o in (math.inf, -math.inf, math.nan)]
    for enc in bad:
        assert call(0, 2, w, h, enc) == -1, enc
        assert L.ofdis_last_error()
        with pytest.raises(gpu.OfdisError):
            gpu.encode(np.zeros(4, _f32), enc)
    # scale and offset are ignored by the float types
    assert call(0, 2, w, h, gpu.Encoding(gpu.ENC_F16, math.nan, math.inf)) == 0
    assert call(0, 2, w, h, gpu.Encoding(gpu.ENC_F32, 0.0, math.nan)) == 0
    gpu.check(L.ofdis_sync(None))
    b.close()
