"""Numpy model of the motion-compensated temporal filter of include/ofdis.h (ofdis_temporal_filter,
ofdis_batch_temporal_filter): the header's definition operation by operation in float32, one rounding at a time.  Needs numpy
only (no GPU, no library): the tests compare the kernels against `temporal_filter_ref` bit for bit.

    from of_dis_amd import temporal
    out, support = temporal.temporal_filter_ref(frames, flow_fw, flow_rev, mask_fw, mask_rev, wn=1.0, tau=24.0)
    both = support == temporal.SUPPORT_PREV | temporal.SUPPORT_NEXT               # pixels averaged over three frames
"""
import numpy as np

SUPPORT_PREV, SUPPORT_NEXT = 1, 2  # bits of `support`: frame f-1 / frame f+1 entered the average with a weight > 0
FB_CONSISTENT = 0  # include/ofdis.h: OFDIS_FB_CONSISTENT (capi.FB_CONSISTENT)

_f32 = np.float32


def inside(px, py, w, h):
    """0 <= px <= w-1 and 0 <= py <= h-1 (NaN: False)"""
    with np.errstate(invalid="ignore"):
        return (px >= _f32(0)) & (px <= _f32(w - 1)) & (py >= _f32(0)) & (py <= _f32(h - 1))


def sample(I, px, py):
    """I [h][w][noc] uint8 sampled bilinearly at the positions (px, py) INSIDE the image, float32 [n] each: [n][noc] float32
    (the expression of ofdis_interpolate)"""
    h, w, _ = I.shape
    n = px.shape
    if w > 1:
        x0 = np.minimum(np.floor(px).astype(np.int64), w - 2)
        ax = px - x0.astype(_f32)
    else:
        x0, ax = np.zeros(n, np.int64), np.zeros(n, _f32)
    if h > 1:
        y0 = np.minimum(np.floor(py).astype(np.int64), h - 2)
        ay = py - y0.astype(_f32)
    else:
        y0, ay = np.zeros(n, np.int64), np.zeros(n, _f32)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    one = _f32(1)
    bx, by = (one - ax)[:, None], (one - ay)[:, None]
    ax, ay = ax[:, None], ay[:, None]
    If = I.astype(_f32)
    r = (If[y0, x0] * bx + If[y0, x1] * ax) * by + (If[y1, x0] * bx + If[y1, x1] * ax) * ay
    assert r.dtype == _f32
    return r


def candidate(c, J, F, M, wn, tau):
    """One neighbour of one frame: c [h][w][noc] float32 (the frame itself), J [h][w][noc] uint8 (the neighbour), F [h][w][2]
    float32 (the flow from the frame to J), M [h][w] uint8 or None -> (w [h][w], s [h][w][noc]) float32"""
    h, w, noc = c.shape
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    with np.errstate(all="ignore"):
        px, py = xs.astype(_f32) + F[..., 0], ys.astype(_f32) + F[..., 1]
    valid = inside(px, py, w, h)
    if M is not None:
        valid &= M == FB_CONSISTENT
    wgt, s = np.zeros((h, w), _f32), np.zeros((h, w, noc), _f32)
    if valid.any():
        sv = sample(J, px[valid], py[valid])
        d = np.abs(sv - c[valid]).max(axis=1)
        with np.errstate(over="ignore", under="ignore"):
            g = np.fmax(_f32(1) - d / _f32(tau), _f32(0))
        wgt[valid], s[valid] = _f32(wn) * g, sv
        assert d.dtype == _f32 and g.dtype == _f32
    return wgt, s


def temporal_filter_ref(frames, flow_fw, flow_rev, mask_fw=None, mask_rev=None, wn=1.0, tau=np.inf):
    """frames [npairs + 1][h][w] (gray) or [npairs + 1][h][w][3] uint8, flow_fw / flow_rev [npairs][h][w][2] float32 (frame k ->
    k + 1 and frame k + 1 -> k), mask_fw / mask_rev [npairs][h][w] uint8 codes or None (all consistent), 0 <= wn <= 1, tau +inf
    or a positive normal float -> (out, the shape of frames, uint8; support [npairs + 1][h][w] uint8), the arrays
    ofdis_temporal_filter writes."""
    frames = np.asarray(frames, np.uint8)
    flow_fw, flow_rev = np.asarray(flow_fw, _f32), np.asarray(flow_rev, _f32)
    npairs, h, w = flow_fw.shape[:3]
    gray = frames.ndim == 3
    I = frames[..., None] if gray else frames
    assert I.shape[:3] == (npairs + 1, h, w) and flow_rev.shape == flow_fw.shape == (npairs, h, w, 2), (frames.shape, flow_fw.shape)
    assert 0.0 <= wn <= 1.0 and tau >= np.finfo(_f32).tiny, (wn, tau)
    out, support = np.empty_like(I), np.empty((npairs + 1, h, w), np.uint8)
    zero_w, zero_s = np.zeros((h, w), _f32), np.zeros(I.shape[1:], _f32)
    one, half = _f32(1), _f32(0.5)
    for f in range(npairs + 1):
        c = I[f].astype(_f32)
        wn_, sn = (candidate(c, I[f + 1], flow_fw[f], None if mask_fw is None else np.asarray(mask_fw)[f], wn, tau)
                   if f < npairs else (zero_w, zero_s))
        wp, sp = (candidate(c, I[f - 1], flow_rev[f - 1], None if mask_rev is None else np.asarray(mask_rev)[f - 1], wn, tau)
                  if f > 0 else (zero_w, zero_s))
        num = (c + wp[..., None] * sp) + wn_[..., None] * sn
        den = (one + wp) + wn_
        r = np.floor(num / den[..., None] + half)
        assert r.dtype == _f32
        out[f] = np.clip(r.astype(np.int64), 0, 255).astype(np.uint8)
        support[f] = np.where(wp > 0, SUPPORT_PREV, 0) | np.where(wn_ > 0, SUPPORT_NEXT, 0)
    return (out[..., 0] if gray else out), support
