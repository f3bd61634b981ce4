"""What the tests of the camera models share (tests/test_gpu_gmotion.py: 6 parameters; tests/test_gpu_projective.py: 8;
tests/test_gpu_launch_limits.py through the former; the two *_abi.py): the generated cases, the comparisons, one row per model order naming its
calls, and the checks both orders take -- each written once with the order as its first argument and run by a test of either
module under that module's own name and cases.  Conditions that hold for one order only are guarded by the order."""
import collections
import functools

import numpy as np

from of_dis_amd import capi, gmotion
from seq_products import assert_same_bits, run_context, smooth_clip

_f32 = np.float32
JUST_ABOVE = np.nextafter(_f32(4096.0), _f32(np.inf))

# A model order: `fit` / `compensate` name the binding's calls (of_dis_amd.capi and, by the same names, capi.Batch) and, with
# _ref appended, the numpy definition's; fit_symbol / compensate_symbol the C functions (<fit_symbol>_work_bytes sizes the work
# buffer); alone_thresh the threshold of the either-output check (8 parameters: at 1 px the few valid +-4096 flows of that case
# leave the fit no inlier)
Order = collections.namedtuple("Order", "nparam fit compensate fit_symbol compensate_symbol alone_thresh")
ORDERS = {6: Order(6, "global_motion", "motion_compensate", "ofdis_global_motion", "ofdis_motion_compensate", 1.0),
          8: Order(8, "projective_motion", "projective_compensate", "ofdis_projective_motion", "ofdis_projective_compensate", 3.0)}


def fit_ref(order, *args, **kw):
    return getattr(gmotion, ORDERS[order].fit + "_ref")(*args, **kw)


def compensate_ref(order, *args, **kw):
    return getattr(gmotion, ORDERS[order].compensate + "_ref")(*args, **kw)


def fit(on, order, *args, **kw):
    """the fit of the order on `on`: the gpu fixture (standalone) or a Batch"""
    return getattr(on, ORDERS[order].fit)(*args, **kw)


def compensate(on, order, *args, **kw):
    return getattr(on, ORDERS[order].compensate)(*args, **kw)


def assert_fit_equal(got, want, what):
    assert_same_bits(got[0], want[0], what + ", models")
    assert_same_bits(got[1], want[1], what + ", stats")


def assert_compensated_equal(got, want, what):
    assert_same_bits(got[0], want[0], what + ", residual")
    assert_same_bits(got[1], want[1], what + ", label")


@functools.lru_cache(maxsize=None)
def _random_case(n, w, h, kind):
    """npairs = n.  "smooth": an affine camera flow of a few pixels per pair plus noise of 0.3 px, a fifth of the pixels with
    flows of 3 px of their own (what the gate removes) and some that stay put.  "wild": the same with large, infinite, NaN
    (default, with a payload, negative), image-sized values and values of exactly +-4096 and just above mixed in, as _random_case
    of tests/test_gpu_tfilter.py mixes them.  Masks with all three codes."""
    rng = np.random.default_rng(w * 1000 + h * 10 + 100 * n + (5 if kind == "wild" else 0))
    F = np.empty((n, h, w, 2), _f32)
    for k in range(n):
        a = rng.normal(0.0, 1.0, 6) * np.array([3.0, 0.02, 0.02, 3.0, 0.02, 0.02])
        F[k] = (gmotion.model_flow(a, w, h) + rng.normal(0.0, 0.3, (h, w, 2))).astype(_f32)
    own = rng.random((n, h, w)) < 0.2
    F[own] = (rng.standard_normal((int(own.sum()), 2)) * 3).astype(_f32)
    F[rng.random((n, h, w)) < 0.05] = 0.0
    if kind == "wild":
        pick = rng.random((n, h, w, 2))
        F[pick < 0.04] = (rng.standard_normal(int((pick < 0.04).sum())) * 1e4).astype(_f32)
        F[(pick >= 0.04) & (pick < 0.05)] = np.inf
        F[(pick >= 0.05) & (pick < 0.06)] = -np.inf
        F[(pick >= 0.06) & (pick < 0.07)] = np.nan
        F[(pick >= 0.07) & (pick < 0.08)] = np.array([0x7FC12345], np.uint32).view(_f32)[0]
        F[(pick >= 0.08) & (pick < 0.09)] = np.array([0xFFC00001], np.uint32).view(_f32)[0]
        sized = (pick >= 0.09) & (pick < 0.10)
        F[sized] = (rng.uniform(-2, 2, int(sized.sum())) * max(w, h)).astype(_f32)
        F[(pick >= 0.130) & (pick < 0.133)] = 4096.0      # (rare: a valid flow of 4096 px pulls the whole fit)
        F[(pick >= 0.133) & (pick < 0.136)] = -4096.0
        F[(pick >= 0.14) & (pick < 0.15)] = JUST_ABOVE
        F[(pick >= 0.15) & (pick < 0.16)] = -JUST_ABOVE
    M = rng.integers(0, 3, (n, h, w), dtype=np.uint8)
    M[rng.random((n, h, w)) < 0.5] = 0
    return F, M


def _keep_only(shape, sel):
    mask = np.full(shape, 1, np.uint8)
    mask[sel] = 0
    return mask


# ------------------------------------------------------------------ checks both orders take
def check_either_output_alone_in_place_and_no_stats(gpu, order):
    t = ORDERS[order].alone_thresh
    flow, mask = _random_case(3, 37, 11, "wild")
    models, _ = fit_ref(order, flow, mask, rounds=2, thresh=t)
    want = compensate_ref(order, flow, models, mask, thresh=t)
    assert np.isnan(want[0]).any() and np.isinf(want[0]).any() and len(np.unique(want[1])) == 3
    res, none = compensate(gpu, order, flow, models, mask, thresh=t, label=False)
    assert none is None
    assert_same_bits(res, want[0], "label = NULL")
    none, label = compensate(gpu, order, flow, models, mask, thresh=t, residual=False)
    assert none is None
    assert_same_bits(label, want[1], "residual = NULL")
    for w, h in ((37, 11), (64, 16)):   # 4-byte and 16-byte stores over the array they were read from
        flow, mask = _random_case(3, w, h, "wild")
        models, _ = fit_ref(order, flow, mask, rounds=2, thresh=1.0)
        assert_compensated_equal(compensate(gpu, order, flow, models, mask, thresh=1.0, in_place=True),
                                 compensate_ref(order, flow, models, mask, thresh=1.0), f"residual aliases flow, {w}x{h}")
    # stats = NULL: the same models
    flow, mask = _random_case(3, 64, 16, "smooth")
    got, none = fit(gpu, order, flow, mask, rounds=3, thresh=1.0, stats=False)
    assert none is None
    assert_same_bits(got, fit_ref(order, flow, mask, rounds=3, thresh=1.0)[0], "stats = NULL")


def check_more_pairs_than_xcds(gpu, order):
    """10 pairs: the pair-to-XCD mapping with its padded last group, every pair with its own records and its own model"""
    for w, h in ((33, 7), (300, 70)):
        flow, mask = _random_case(10, w, h, "smooth")
        want = fit_ref(order, flow, mask, rounds=3, thresh=1.0)
        assert len({m.tobytes() for m in want[0]}) == 10
        if order == 8:
            assert (want[1][:, 2] == 8).sum() >= 5
        assert_fit_equal(fit(gpu, order, flow, mask, rounds=3, thresh=1.0), want, f"10 pairs {w}x{h}")
        assert_compensated_equal(compensate(gpu, order, flow, want[0], mask, thresh=1.0),
                                 compensate_ref(order, flow, want[0], mask, thresh=1.0), f"10 pairs {w}x{h}")


def check_unaligned_outputs(gpu, order, w, h):
    """the residual one element (4 bytes) and the labels one byte into their buffers: the same bytes as the aligned call, and the
    guard bytes around both stay"""
    npairs = 3
    flow, mask = _random_case(npairs, w, h, "wild")
    models, _ = fit_ref(order, flow, mask, rounds=2, thresh=1.0)
    want = compensate_ref(order, flow, models, mask, thresh=1.0)
    rbytes, lbytes = flow.nbytes, npairs * h * w
    devs = [gpu.Dev(x) for x in (flow, mask, models)]
    call = getattr(gpu.lib(), ORDERS[order].compensate_symbol)
    for roff, loff in ((260, 257), (264, 258), (272, 260)):   # residual 4 / 8 / 16-byte aligned, labels 1 / 2 / 4-byte aligned
        dr = gpu.Dev(np.full(rbytes + 2 * roff, 0xAB, np.uint8))
        dl = gpu.Dev(np.full(lbytes + 2 * loff, 0xAB, np.uint8))
        gpu.check(call(devs[0].ptr, devs[1].ptr, devs[2].ptr, npairs, w, h, 1.0, dr.ptr + roff, dl.ptr + loff, None))
        gpu.check(gpu.lib().ofdis_sync(None))
        r, l = dr.get((rbytes + 2 * roff,), np.uint8), dl.get((lbytes + 2 * loff,), np.uint8)
        for buf, off, n in ((r, roff, rbytes), (l, loff, lbytes)):
            assert (buf[:off] == 0xAB).all() and (buf[off + n:] == 0xAB).all(), (roff, loff)
        assert_same_bits(r[roff:roff + rbytes].copy().view(_f32).reshape(flow.shape), want[0], f"residual at offset {roff}")
        assert_same_bits(l[loff:loff + lbytes].reshape(npairs, h, w), want[1], f"labels at offset {loff}")


def check_fused_matches_standalone(gpu, order, fits, kind, noc, opp, w, h, n, first, count, pipeline, contract, alpha, beta):
    """fb_check = 0 against the standalone calls on upsample_frames' output with mask NULL; fb_check = 1 (contexts with the
    reverse direction) against them on out_fw and mask_fw of upsample_bidir.  fits: the keywords of every fit to run"""
    clip = smooth_clip(w, h, noc, n + 1)
    b, devs = run_context(gpu, clip, kind, opp, contract, pipeline)
    fused = []
    try:
        bytes_before = b.device_bytes()
        for fb in ((0, 1) if kind != "plain" else (0,)):
            for kw in fits:
                got = fit(b, order, w, h, fb_check=fb, first=first, count=count, alpha=alpha, beta=beta, **kw)
                comp = compensate(b, order, got[0], w, h, thresh=kw["thresh"], fb_check=fb, first=first, count=count, alpha=alpha,
                                  beta=beta)
                fused.append((fb, kw, got, comp))
        # the slab belongs to the context: allocated once, counted from then on
        slab = b.device_bytes() - bytes_before
        assert slab >= getattr(gpu.lib(), ORDERS[order].fit_symbol + "_work_bytes")(n, w, h) > 0
        plain = b.upsample_frames(first, count, w, h)
        fw, mf = b.upsample_bidir(w, h, alpha, beta, first=first, count=count, outputs=(True, False, True, False))[0::2] \
            if kind != "plain" else (None, None)
        assert b.device_bytes() - bytes_before == slab
    finally:
        b.close()
    for fb, kw, got, comp in fused:
        flow, mask = (fw, mf) if fb else (plain, None)
        what = f"fb_check {fb}, " + ", ".join(f"{k} {v}" for k, v in kw.items())
        standalone = fit(gpu, order, flow, mask, **kw)
        assert_fit_equal(got, standalone, "fused vs standalone, " + what)
        assert_compensated_equal(comp, compensate(gpu, order, flow, standalone[0], mask, thresh=kw["thresh"]),
                                 "fused vs standalone, " + what)
        if count <= 3:
            assert_fit_equal(standalone, fit_ref(order, flow, mask, **kw), "standalone vs the definition, " + what)
        if not (fb and alpha == 0.0 and beta == 0.0):   # something was fitted in the comparison
            assert (standalone[1][:, 0] > 0).all()
            if order == 8:
                assert (standalone[1][:, 2] == 8).all()
    if kind != "plain":
        assert_same_bits(fw, plain, "upsample_bidir's forward flow is upsample_frames'")
        if alpha == 0.0 and beta == 0.0:   # (a test nothing but an exact round trip passes: most pixels are masked here)
            assert (mf != 0).mean() > 0.5
        else:
            assert (mf != 0).mean() < 0.5


# ------------------------------------------------------------------ the argument checks of the standalone calls (no device work)
class Host:
    """host stand-ins for a 2-pair 8x4 case with models of nparam doubles: every call returns before it would launch"""

    def __init__(self, nparam, w=8, h=4, npairs=2):
        self.nparam = nparam
        self.flow = np.zeros((npairs, h, w, 2), _f32)
        self.mask = np.zeros((npairs, h, w), np.uint8)
        self.models = np.zeros((npairs, nparam), np.float64)
        self.stats = np.zeros((npairs, 3), np.int64)
        self.work = np.zeros(4096, np.int64)
        self.residual = np.zeros((npairs, h, w, 2), _f32)
        self.label = np.zeros((npairs, h, w), np.uint8)


def _p(array, on=True):
    return array.ctypes.data if on else None


def host_fit(hb, flow=True, models=True, work=True, work_bytes=None, work_off=0, npairs=2, w=8, h=4, model=1, rounds=3,
             thresh=1.0):
    """the standalone fit of hb's order (`model` goes to the 6-parameter one only)"""
    wb = hb.work.nbytes - 8 if work_bytes is None else work_bytes
    wp = hb.work.ctypes.data + work_off if work else None
    return getattr(capi.lib(), ORDERS[hb.nparam].fit_symbol)(_p(hb.flow, flow), _p(hb.mask), npairs, w, h,
                                                             *([model] if hb.nparam == 6 else []), rounds, thresh,
                                                             _p(hb.models, models), _p(hb.stats), wp, wb, None)


def host_compensate(hb, flow=True, models=True, residual=True, label=True, npairs=2, w=8, h=4, thresh=1.0):
    return getattr(capi.lib(), ORDERS[hb.nparam].compensate_symbol)(_p(hb.flow, flow), _p(hb.mask), _p(hb.models, models), npairs,
                                                                    w, h, thresh, _p(hb.residual, residual), _p(hb.label, label),
                                                                    None)


BAD_SIZES = [(0, 8, 4), (-1, 8, 4), (2, 0, 4), (2, 8, 0), (2, -8, 4), (2, 1 << 16, 1 << 16), (2, 8193, 4), (2, 8, 8193)]
