"""-m gpu: bidirectional flow (ofdis_batch_create_ex with OFDIS_BATCH_REVERSE), the forward-backward consistency test
(ofdis_fb_check) and the one-launch full-resolution output of both directions with both masks (ofdis_batch_upsample_bidir).

The reverse flow of a pair (A, B) is DEFINED as the forward flow a plain context of the same size computes for (B, A): every
comparison here is bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gen_synth
from common import assert_bits_equal, synth_case
from of_dis_amd.params import oppoint, padded_size
from seq_products import check_levels, fill_u8, levels

pytestmark = pytest.mark.gpu
_f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ helpers
def _u8_frames(w, h, noc, seeds):
    pairs = [gen_synth.make_pair(w, h, s, noc)[:2] for s in seeds]
    return np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])


def _fill_host(b, cases, swap=False):
    """cases: list of (pa, pb) host pyramids per frame ([img, dx, dy] lists over levels)"""
    for k, (pa, pb) in enumerate(cases):
        if swap:
            pa, pb = pb, pa
        b.upload(k, pa[0], pa[1], pa[2], pb[0])
        b.upload_b_gradients(k, pb[1], pb[2])


def _run_three(gpu, p, n, fill, data):
    """(reverse context: forward levels, reverse levels), plain context on (A, B), plain context on (B, A)"""
    rb = gpu.Batch(p, n, reverse=True)
    pf = gpu.Batch(p, n)
    ps = gpu.Batch(p, n)
    if fill == "u8":
        ia, ib, w, h = data
        fill_u8(gpu, rb, ia, ib, w, h)
        fill_u8(gpu, pf, ia, ib, w, h)
        fill_u8(gpu, ps, ib, ia, w, h)
    else:
        _fill_host(rb, data)
        _fill_host(pf, data)
        _fill_host(ps, data, swap=True)
    for b in (rb, pf, ps):
        b.run()
    out = (levels(rb, p), levels(rb, p, "reverse"), levels(pf, p), levels(ps, p))
    for b in (rb, pf, ps):
        b.close()
    return out


# (noc, op, usefbcon, tv, nframes, fill, width, height)
REV_CASES = [
    pytest.param(1, 2, 0, 1, 3, "host", 256, 112, id="gray-op2-tv-n3-host"),
    pytest.param(1, 2, 0, 0, 1, "u8", 256, 112, id="gray-op2-notv-n1-u8"),
    pytest.param(1, 1, 0, 0, 3, "u8", 256, 112, id="gray-op1-n3-u8"),
    pytest.param(1, 3, 0, 1, 1, "host", 320, 240, id="gray-op3-n1-host"),
    pytest.param(1, 4, 0, 1, 1, "u8", 256, 112, id="gray-op4-n1-u8"),
    pytest.param(1, 2, 1, 1, 3, "host", 256, 112, id="gray-op2-fb-tv-n3-host"),
    pytest.param(1, 2, 1, 0, 3, "u8", 256, 112, id="gray-op2-fb-notv-n3-u8"),
    pytest.param(3, 2, 0, 1, 3, "u8", 256, 112, id="rgb-op2-tv-n3-u8"),
    pytest.param(3, 2, 0, 0, 1, "host", 256, 112, id="rgb-op2-notv-n1-host"),
    pytest.param(3, 3, 1, 1, 1, "host", 320, 240, id="rgb-op3-fb-n1-host"),
    pytest.param(3, 2, 1, 1, 3, "u8", 256, 112, id="rgb-op2-fb-tv-n3-u8"),
    # more frames than the small-batch mappings of the fused TV kernel take (cross-CU <= 768, multi-wave <= 512 groups):
    # the throughput mapping over strips
    pytest.param(1, 2, 0, 1, 800, "u8", 256, 112, id="gray-op2-tv-n800-u8-strips"),
]


@pytest.mark.parametrize("contract", [0, 1], ids=["exact", "fused"])
@pytest.mark.parametrize("noc,opp,fb,tv,n,fill,w,h", REV_CASES)
def test_reverse_equals_swapped_forward(gpu, orc, contract, noc, opp, fb, tv, n, fill, w, h):
    """Every level of frame k's reverse flow == the forward flow of a plain context (same nframes, params, contract) on
    (B_k, A_k); the forward flow of the REVERSE context == a plain context's.  Exact contract, usefbcon 0: also the
    oracle's restatement of the swapped pair."""
    p = oppoint(opp, w, h, noc=noc, usetvref=tv).copy(usefbcon=fb)
    p.width, p.height = padded_size(w, h, p.sc_f)
    seeds = [3100 + 7 * k for k in range(min(n, 3))]
    order = [k % len(seeds) for k in range(n)]
    if fill == "u8":
        ia, ib = _u8_frames(w, h, noc, seeds)
        ia, ib = ia[order], ib[order]
        data = (ia, ib, w, h)
    else:
        pyr = []
        for s in seeds:
            _, pa, pb, _, _ = synth_case(w, h, s, noc, opp, tv)
            pyr.append((pa, pb))
        data = [pyr[k] for k in order]
    old = gpu.set_tuning(contract=contract)
    try:
        fwd, rev, plain_fwd, plain_swp = _run_three(gpu, p, n, fill, data)
    finally:
        gpu.restore_tuning(old)
    check_levels(fwd, plain_fwd, "forward flow of the REVERSE context vs a plain context")
    check_levels(rev, plain_swp, "reverse flow vs a plain context on the swapped pairs")
    assert not np.array_equal(rev[p.sc_l], fwd[p.sc_l])
    if contract == 0 and fb == 0:  # the restatement does not cover usefbcon
        for k in range(len(seeds)):
            if fill == "u8":
                pa, pb = orc.build_pyramid(p, ia[k]), orc.build_pyramid(p, ib[k])
            else:
                pa, pb = data[k]
            ref = orc.flow(p, pb[0], pb[1], pb[2], pa[0])
            assert_bits_equal(rev[p.sc_l][k], ref, f"reverse flow of frame {k} vs the oracle on (B, A)")


def test_reverse_across_tv_variants(gpu, orc, tv_variant):
    """Exact contract over every mapping of the fused TV kernel (tests/conftest.py: tv_variant)."""
    w, h = 1024, 436
    cases = [synth_case(w, h, 4100 + k, 1, 2, 1) for k in range(2)]
    p = cases[0][0]
    data = [(c[1], c[2]) for c in (cases[0], cases[1], cases[1], cases[0])]
    fwd, rev, plain_fwd, plain_swp = _run_three(gpu, p, 4, "host", data)
    check_levels(fwd, plain_fwd, f"{tv_variant}: forward")
    check_levels(rev, plain_swp, f"{tv_variant}: reverse")
    for k in range(2):
        _, pa, pb, _, _ = cases[k]
        assert_bits_equal(rev[p.sc_l][k], orc.flow(p, pb[0], pb[1], pb[2], pa[0]), f"{tv_variant}: oracle, frame {k}")


@pytest.mark.parametrize("how,arg", [("pipeline", 2), ("pipeline", 3), ("pipeline", 4), ("graph", 1), ("graph", -1)])
def test_reverse_pipelined_and_graph(gpu, how, arg):
    """Sub-batches on internal streams (ragged: 7 frames) and launch-graph replay: both directions identical to the plain
    single-stream run, over two consecutive passes (the second replays the graph / overlaps the first)."""
    w, h = 1024, 436
    cases = [synth_case(w, h, 4200 + k, 1, 2, 1) for k in range(3)]
    p = cases[0][0]
    data = [(cases[k][1], cases[k][2]) for k in (0, 1, 2, 2, 1, 0, 1)]
    _, _, plain_fwd, plain_swp = _run_three(gpu, p, 7, "host", data)
    b = gpu.Batch(p, 7, reverse=True)
    _fill_host(b, data)
    if how == "pipeline":
        b.set_pipeline(arg)
    else:
        b.set_graph(arg)
    for rep in range(2):
        b.run()
        if how == "pipeline":
            b.run()  # two passes in flight before anything joins
        assert_bits_equal(b.download_all(), plain_fwd[p.sc_l], f"{how} {arg}, pass {rep}: forward")
        assert_bits_equal(b.download_all_reverse(), plain_swp[p.sc_l], f"{how} {arg}, pass {rep}: reverse")
    assert_bits_equal(b.download_reverse(4), plain_swp[p.sc_l][4], "ofdis_batch_download_reverse")
    b.close()


def test_reverse_warm_start(gpu):
    """set_initflow_reverse(X) == a swapped-pair forward run with initflow = X; the forward direction stays cold; NULL
    switches it off again; a captured launch graph is rebuilt when the reverse warm start changes."""
    w, h = 1024, 436
    cases = [synth_case(w, h, 4300 + k, 1, 2, 1) for k in range(2)]
    p = cases[0][0]
    data = [(c[1], c[2]) for c in cases]
    n = len(data)
    _, _, plain_fwd, plain_swp = _run_three(gpu, p, n, "host", data)
    cw, ch = p.level_size(p.sc_f)
    init = (np.random.default_rng(77).standard_normal((n, ch // 2, cw // 2, 2)) * 0.7).astype(_f32)
    dinit = gpu.Dev(init)
    ps = gpu.Batch(p, n)
    _fill_host(ps, data, swap=True)
    ps.set_initflow(dinit.ptr)
    ps.run()
    warm = ps.download_all()
    ps.close()
    assert not np.array_equal(warm, plain_swp[p.sc_l])
    b = gpu.Batch(p, n, reverse=True)
    b.set_graph(1)
    _fill_host(b, data)
    b.run()
    assert_bits_equal(b.download_all_reverse(), plain_swp[p.sc_l], "cold")
    b.set_initflow_reverse(dinit.ptr)
    for rep in range(2):
        b.run()
        assert_bits_equal(b.download_all_reverse(), warm, f"reverse warm start, pass {rep}")
        assert_bits_equal(b.download_all(), plain_fwd[p.sc_l], f"forward stays cold, pass {rep}")
    b.set_initflow_reverse(None)
    b.run()
    assert_bits_equal(b.download_all_reverse(), plain_swp[p.sc_l], "reverse warm start off again")
    b.close()


# ------------------------------------------------------------------ ofdis_fb_check
def fb_check_ref(flow, other, alpha=0.01, beta=0.5):
    """float32 numpy restatement of include/ofdis.h: ofdis_fb_check (every operation separately rounded)."""
    flow, other = np.asarray(flow, _f32), np.asarray(other, _f32)
    n, h, w, _ = flow.shape
    a, bt = _f32(alpha), _f32(beta)
    one = _f32(1)
    out = np.empty((n, h, w), np.uint8)
    X = np.broadcast_to(np.arange(w, dtype=_f32)[None, :], (h, w))
    Y = np.broadcast_to(np.arange(h, dtype=_f32)[:, None], (h, w))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(n):
            u, v = flow[k, ..., 0], flow[k, ..., 1]
            xb, yb = X + u, Y + v
            inside = (xb >= 0) & (xb <= _f32(w - 1)) & (yb >= 0) & (yb <= _f32(h - 1))
            xs, ys = np.where(inside, xb, _f32(0)), np.where(inside, yb, _f32(0))
            if w > 1:
                x0 = np.minimum(np.floor(xs).astype(np.int64), w - 2)
                ax = xs - x0.astype(_f32)
            else:
                x0, ax = np.zeros((h, w), np.int64), np.zeros((h, w), _f32)
            if h > 1:
                y0 = np.minimum(np.floor(ys).astype(np.int64), h - 2)
                ay = ys - y0.astype(_f32)
            else:
                y0, ay = np.zeros((h, w), np.int64), np.zeros((h, w), _f32)
            x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
            R = other[k]
            bx, by = one - ax, one - ay
            r = (R[y0, x0] * bx[..., None] + R[y0, x1] * ax[..., None]) * by[..., None] + \
                (R[y1, x0] * bx[..., None] + R[y1, x1] * ax[..., None]) * ay[..., None]
            ru, rv = r[..., 0], r[..., 1]
            du, dv = u + ru, v + rv
            lhs = du * du + dv * dv
            rhs = a * ((u * u + v * v) + (ru * ru + rv * rv)) + bt
            code = np.where(lhs <= rhs, 0, 1).astype(np.uint8)
            out[k] = np.where(inside, code, 2)
    return out


@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (1, 1, 2), (1, 2, 1), (2, 2, 2), (3, 7, 5), (2, 37, 61), (1, 1, 33), (1, 29, 1),
                                   (4, 128, 96)])
@pytest.mark.parametrize("alpha,beta", [(0.01, 0.5), (0.0, 0.0), (0.3, 2.0)])
def test_fb_check_random_flows(gpu, n, h, w, alpha, beta):
    rng = np.random.default_rng(n * 1000 + h * 31 + w)
    scale = max(1.0, 0.3 * min(w, h))
    f = (rng.standard_normal((n, h, w, 2)) * scale).astype(_f32)
    # half the pixels: the other flow is close to the negated flow at the target (mostly consistent)
    o = (-f + rng.standard_normal((n, h, w, 2)).astype(_f32) * _f32(0.2)).astype(_f32)
    for a, b in ((f, o), (o, f)):
        got = gpu.fb_check(a, b, alpha, beta)
        want = fb_check_ref(a, b, alpha, beta)
        assert np.array_equal(got, want), (np.argwhere(got != want)[:5], alpha, beta)
    assert gpu.fb_check(f, o, alpha, beta).max() <= 2


def test_fb_check_hand_built_cases(gpu):
    """lhs == rhs exactly, targets exactly on W-1 / H-1 and just past them, NaN, -0.0."""
    h, w = 5, 6
    f = np.zeros((1, h, w, 2), _f32)
    o = np.zeros((1, h, w, 2), _f32)
    nxt = np.nextafter
    # (0,0): u = v = 0 onto the other flow (0.5, 0) -> lhs = 0.25; alpha 0, beta 0.25 -> lhs == rhs: consistent
    o[0, 0, 0] = (0.5, 0.0)
    # (1,0): the same with beta just below -> inconsistent (beta chosen per call below; pixel (1,0) points at (0,0))
    f[0, 0, 1] = (-1.0, 0.0)
    # target exactly on W-1 / H-1 (inside), and one ulp past (outside)
    f[0, 2, 0] = (w - 1, h - 1 - 2)
    f[0, 2, 1] = (nxt(_f32(w - 2), _f32(100)), 0.0)          # 1 + (4 + 2^-21) = 5 + 2^-21, exact
    f[0, 3, 0] = (0.0, _f32(1) + _f32(2.0 ** -21))            # 3 + (1 + 2^-21) = 4 + 2^-21, exact
    f[0, 4, 0] = (0.0, _f32(h - 1 - 4))
    f[0, 1, 0] = (-(2.0 ** -20), 0.0)                  # just left of x = 0: outside
    f[0, 1, 1] = (np.nan, 0.0)
    f[0, 1, 2] = (0.0, np.nan)
    f[0, 1, 3] = (-0.0, -0.0)
    f[0, 1, 4] = (-4.0, -1.0)                        # exactly onto (0, 0)
    got = gpu.fb_check(f, o, 0.0, 0.25)
    assert np.array_equal(got, fb_check_ref(f, o, 0.0, 0.25))
    assert got[0, 0, 0] == 0, "lhs == rhs is consistent"
    assert got[0, 2, 0] != 2 and got[0, 4, 0] != 2, "a target exactly on W-1 / H-1 is inside"
    assert got[0, 2, 1] == 2 and got[0, 3, 0] == 2 and got[0, 1, 0] == 2, "one ulp past the border is outside"
    assert got[0, 1, 1] == 2 and got[0, 1, 2] == 2, "NaN is outside"
    assert got[0, 1, 3] == 0
    below = float(nxt(_f32(0.25), _f32(0)))
    got2 = gpu.fb_check(f, o, 0.0, below)
    assert np.array_equal(got2, fb_check_ref(f, o, 0.0, below))
    assert got2[0, 0, 0] == 1 and got2[0, 0, 1] == 1 and got2[0, 1, 4] == 1
    # -0.0 flows everywhere: the same mask as +0.0
    z = np.zeros((2, 3, 4, 2), _f32)
    assert np.array_equal(gpu.fb_check(-z, z), gpu.fb_check(z, -z))
    assert not gpu.fb_check(z, z).any()


@pytest.mark.parametrize("t", [(3.0, 0.0), (0.0, -2.0), (2.5, -1.25), (-7.75, 4.0)])
def test_fb_check_opposite_translations(gpu, t):
    """Constant flow t one way and -t the other: OUTSIDE exactly on the border band of ceil(|t|) columns / rows the shift
    leaves the image, CONSISTENT everywhere else."""
    h, w = 40, 52
    f = np.empty((1, h, w, 2), _f32)
    f[...] = t
    got = gpu.fb_check(f, -f)[0]
    X, Y = np.meshgrid(np.arange(w), np.arange(h))
    tx, ty = t
    cx, cy = int(np.ceil(abs(tx))), int(np.ceil(abs(ty)))
    out_x = (X >= w - cx) if tx > 0 else (X < cx)
    out_y = (Y >= h - cy) if ty > 0 else (Y < cy)
    expect = np.where(out_x | out_y, 2, 0)
    assert np.array_equal(got, expect), np.argwhere(got != expect)[:5]


def test_fb_check_moving_square(gpu):
    """A square moving d pixels right over a static background: the background it covers in the second image (a band of d
    columns right of the square in the first) is INCONSISTENT in the forward mask, the background it uncovers (d columns
    at its old left edge) in the reverse mask; everything else is CONSISTENT."""
    h, w, x0, y0, S, d = 48, 64, 20, 14, 16, 5
    fw = np.zeros((1, h, w, 2), _f32)
    rv = np.zeros((1, h, w, 2), _f32)
    fw[0, y0:y0 + S, x0:x0 + S] = (d, 0)
    rv[0, y0:y0 + S, x0 + d:x0 + d + S] = (-d, 0)
    mf, mr = gpu.fb_check(fw, rv)[0], gpu.fb_check(rv, fw)[0]
    ef, er = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    ef[y0:y0 + S, x0 + S:x0 + S + d] = 1
    er[y0:y0 + S, x0:x0 + d] = 1
    assert np.array_equal(mf, ef), np.argwhere(mf != ef)[:5]
    assert np.array_equal(mr, er), np.argwhere(mr != er)[:5]


# ------------------------------------------------------------------ ofdis_batch_upsample_bidir
@pytest.mark.parametrize("w,h,opp,noc,n,first,count", [
    (256, 112, 2, 1, 3, 0, None),    # sc_l = 1 (x 2), no crop
    (333, 251, 1, 1, 3, 1, 2),       # odd size: asymmetric crop, sub-range
    (321, 239, 3, 1, 2, 0, 1),       # sc_l = 0 (x 1), odd size, crop
    (250, 110, 2, 3, 3, 2, 1),       # RGB, crop, last frame
    (1024, 436, 2, 1, 2, 0, None),   # the measured geometry: sc_l = 3 (x 8)
])
def test_upsample_bidir(gpu, w, h, opp, noc, n, first, count):
    p = oppoint(opp, w, h, noc=noc)
    p.width, p.height = padded_size(w, h, p.sc_f)
    ia, ib = _u8_frames(w, h, noc, [5100 + k for k in range(n)])
    rb, ps = gpu.Batch(p, n, reverse=True), gpu.Batch(p, n)
    fill_u8(gpu, rb, ia, ib, w, h)
    fill_u8(gpu, ps, ib, ia, w, h)
    rb.run()
    ps.run()
    count = n - first if count is None else count
    fw_ref = rb.upsample_frames(first, count, w, h)
    rev_ref = ps.upsample_frames(first, count, w, h)
    for alpha, beta in ((0.01, 0.5), (0.05, 0.0)):
        fw, rev, mf, mr = rb.upsample_bidir(w, h, alpha, beta, first=first, count=count)
        assert_bits_equal(fw, fw_ref, "forward flow vs ofdis_batch_upsample_frames")
        assert_bits_equal(rev, rev_ref, "reverse flow vs ofdis_batch_upsample_frames of the swapped pairs")
        assert np.array_equal(mf, gpu.fb_check(fw_ref, rev_ref, alpha, beta)), "forward mask vs ofdis_fb_check"
        assert np.array_equal(mr, gpu.fb_check(rev_ref, fw_ref, alpha, beta)), "reverse mask vs ofdis_fb_check"
        assert np.array_equal(mf, fb_check_ref(fw_ref, rev_ref, alpha, beta)), "forward mask vs the numpy restatement"
        assert mf.shape == (count, h, w) and (mf == 0).mean() > 0.3
    # NULL outputs: the others are unaffected
    for sel in ((False, True, False, True), (True, False, True, False), (False, False, True, False), (False, False, False, False)):
        res = rb.upsample_bidir(w, h, first=first, count=count, outputs=sel)
        full = rb.upsample_bidir(w, h, first=first, count=count)
        for r, f, want in zip(res, full, sel):
            if want:
                assert_bits_equal(r, f, f"outputs {sel}") if r.dtype == _f32 else np.testing.assert_array_equal(r, f)
            else:
                assert r is None
    rb.close()
    ps.close()


def test_bidir_error_paths(gpu):
    L = gpu.lib()
    p = oppoint(2, 256, 112)
    import ctypes as C
    h = C.c_void_p()
    assert L.ofdis_batch_create_ex(C.byref(h), C.byref(p.copy(selectmode=2)), 2, 1) == -2  # stereo + REVERSE
    assert L.ofdis_batch_create_ex(C.byref(h), C.byref(p), 2, 2) == -1                     # unknown flag
    assert L.ofdis_batch_create_ex(C.byref(h), C.byref(p), 2, 0x80000001) == -1
    plain = gpu.Batch(p, 2)
    assert not L.ofdis_batch_flow_reverse(plain.h)
    assert not L.ofdis_batch_level_flow_reverse(plain.h, p.sc_l)
    assert L.ofdis_batch_set_initflow_reverse(plain.h, None) == -1
    buf = np.zeros(p.level_size(p.sc_l)[0] * p.level_size(p.sc_l)[1] * 2, _f32)
    assert L.ofdis_batch_download_reverse(plain.h, 0, buf.ctypes.data_as(gpu.FP), None) == -1
    with pytest.raises(gpu.OfdisError):
        plain.upsample_bidir(256, 112)
    assert plain.input_ptr(p.sc_l, 4) is None  # no B gradients without usefbcon or REVERSE
    plain.close()
    rb = gpu.Batch(p, 2, reverse=True)
    assert rb.input_ptr(p.sc_l, 4) and rb.input_ptr(p.sc_f, 5)
    assert L.ofdis_batch_flow_reverse(rb.h) and L.ofdis_batch_level_flow_reverse(rb.h, p.sc_f)
    assert not L.ofdis_batch_level_flow_reverse(rb.h, p.sc_f + 1)
    for a, b in ((-0.01, 0.5), (0.01, -0.5), (float("inf"), 0.5), (0.01, float("nan")), (float("nan"), 0.5)):
        with pytest.raises(gpu.OfdisError):
            rb.upsample_bidir(256, 112, a, b)
        with pytest.raises(gpu.OfdisError):
            gpu.fb_check(np.zeros((1, 4, 4, 2), _f32), np.zeros((1, 4, 4, 2), _f32), a, b)
    with pytest.raises(gpu.OfdisError):
        rb.upsample_bidir(256, 112, first=1, count=2)   # range outside the batch
    with pytest.raises(gpu.OfdisError):
        rb.upsample_bidir(300, 112)                       # larger than the padded size
    rb.close()


def test_flow_images_reverse(gpu, tmp_path):
    """tools/flow_images.py --reverse: the forward .flo is the bytes without --reverse; .rev.flo is the forward .flo of the
    swapped pair; the masks are binary PGMs of the codes; --reverse --stereo is refused."""
    from PIL import Image
    w, h = 200, 150
    ia, ib, _ = gen_synth.make_pair(w, h, 6100, 1)
    pa, pb = str(tmp_path / "a.png"), str(tmp_path / "b.png")
    Image.fromarray(ia).save(pa)
    Image.fromarray(ib).save(pb)
    tool = os.path.join(ROOT, "tools", "flow_images.py")
    run = lambda args: subprocess.run([sys.executable, tool] + args, capture_output=True, text=True, timeout=300)
    o, r, s = str(tmp_path / "fw.flo"), str(tmp_path / "plain.flo"), str(tmp_path / "swapped.flo")
    for args in (["--reverse", pa, pb, o], [pa, pb, r], [pb, pa, s]):
        res = run(args)
        assert res.returncode == 0, (res.stdout, res.stderr)
    assert open(o, "rb").read() == open(r, "rb").read()
    assert open(str(tmp_path / "fw.rev.flo"), "rb").read() == open(s, "rb").read()
    for name in ("fw.mask.pgm", "fw.rev.mask.pgm"):
        data = open(str(tmp_path / name), "rb").read()
        head = b"P5\n%d %d\n2\n" % (w, h)
        assert data.startswith(head) and len(data) == len(head) + w * h
        m = np.frombuffer(data[len(head):], np.uint8)
        assert m.max() <= 2 and (m == 0).mean() > 0.3
    res = run(["--reverse", "--stereo", pa, pb, str(tmp_path / "x.pfm")])
    assert res.returncode != 0 and "stereo" in (res.stderr + res.stdout)
