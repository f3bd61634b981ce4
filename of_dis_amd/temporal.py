"""Numpy model of the motion-compensated temporal filter of include/ofdis.h (ofdis_temporal_filter,
ofdis_batch_temporal_filter): the header's definition operation by operation in float32, one rounding at a time.  Needs numpy
only (no GPU, no library): the tests compare the kernels against `temporal_filter_ref` bit for bit.

    from of_dis_amd import temporal
    out, support = temporal.temporal_filter_ref(frames, flow_fw, flow_rev, mask_fw, mask_rev, wn=1.0, tau=24.0)
    both = support == temporal.SUPPORT_PREV | temporal.SUPPORT_NEXT               # pixels averaged over three frames

and of the filter along flow trajectories over 2R + 1 frames (ofdis_trajectory_filter, ofdis_batch_trajectory_filter), built on
the pieces of of_dis_amd/tracking.py:

    w = temporal.trajectory_weights(2)                                            # flat: [1, 1]
    out, support = temporal.trajectory_filter_ref(frames, flow_fw, flow_rev, w, tau=24.0, fb_check=True)
    nb, nf = temporal.reach(support)                                              # steps back / forward that entered
"""
import numpy as np

from . import tracking

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


# ------------------------------------------------------------------------------------ along trajectories over 2R + 1 frames
TRAJ_MAX_RADIUS = 8  # include/ofdis.h: OFDIS_TRAJ_MAX_RADIUS (capi.TRAJ_MAX_RADIUS)


def trajectory_weights(radius, wn=1.0, sigma=None):
    """w_1 .. w_radius as float32: flat (every w_j = wn), or wn * exp(-j^2 / (2 sigma^2)) rounded to float32"""
    j = np.arange(1, radius + 1, dtype=np.float64)
    w = np.full(radius, float(wn)) if sigma is None else float(wn) * np.exp(-j * j / (2.0 * float(sigma) ** 2))
    return w.astype(_f32)


def reach(support):
    """support of the trajectory filter -> (nb, nf): how many steps back / forward entered the average with a weight > 0"""
    support = np.asarray(support, np.uint8)
    return support >> 4, support & 15


def _walk(I, c, f, forward, flow_fw, flow_rev, weights, tau, fb_check, alpha, beta):
    """one direction of frame f: (w [R][h][w], s [R][h][w][noc]) float32, zero where a step is not reached"""
    npairs, h, w = flow_fw.shape[:3]
    R, noc = len(weights), I.shape[-1]
    wgt, s = np.zeros((R, h, w), _f32), np.zeros((R, h, w, noc), _f32)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    iy, ix = ys.ravel(), xs.ravel()                       # the walks still alive: their pixels ...
    px, py = ix.astype(_f32), iy.astype(_f32)             # ... and where they stand
    cf = c.reshape(-1, noc)
    for j in range(1, R + 1):
        k = f + j - 1 if forward else f - j
        if k < 0 or k >= npairs or ix.size == 0:
            break
        F, O = (flow_fw[k], flow_rev[k]) if forward else (flow_rev[k], flow_fw[k])
        J = I[f + j] if forward else I[f - j]
        u, v = (F[iy, ix, 0], F[iy, ix, 1]) if j == 1 else tracking.bilinear(F, px, py)
        with np.errstate(all="ignore"):
            qx, qy = px + u, py + v
        ok = tracking.inside(qx, qy, w, h)
        if fb_check:
            i = np.flatnonzero(ok)
            ru, rv = tracking.bilinear(O, qx[i], qy[i])
            ok[i] = tracking.consistent(u[i], v[i], ru, rv, alpha, beta)
        iy, ix, px, py = iy[ok], ix[ok], qx[ok], qy[ok]
        if ix.size == 0:
            break
        sv = sample(J, px, py)
        d = np.abs(sv - cf[iy * w + ix]).max(axis=1)
        with np.errstate(over="ignore", under="ignore"):
            g = np.fmax(_f32(1) - d / _f32(tau), _f32(0))
        assert d.dtype == _f32 and g.dtype == _f32
        wgt[j - 1, iy, ix], s[j - 1, iy, ix] = _f32(weights[j - 1]) * g, sv
    return wgt, s


def trajectory_filter_ref(frames, flow_fw, flow_rev, weights, tau=np.inf, fb_check=True, alpha=tracking.FB_ALPHA,
                          beta=tracking.FB_BETA):
    """frames [npairs + 1][h][w] (gray) or [npairs + 1][h][w][3] uint8, flow_fw / flow_rev [npairs][h][w][2] float32 (frame k ->
    k + 1 and frame k + 1 -> k), weights [radius] with 1 <= radius <= TRAJ_MAX_RADIUS and every weight in [0, 1], tau +inf or a
    positive normal float -> (out, the shape of frames, uint8; support [npairs + 1][h][w] uint8 = nf | nb << 4), the arrays
    ofdis_trajectory_filter writes."""
    frames = np.asarray(frames, np.uint8)
    flow_fw, flow_rev = np.asarray(flow_fw, _f32), np.asarray(flow_rev, _f32)
    weights = np.asarray(weights, _f32).ravel()
    npairs, h, w = flow_fw.shape[:3]
    gray = frames.ndim == 3
    I = frames[..., None] if gray else frames
    assert I.shape[:3] == (npairs + 1, h, w) and flow_rev.shape == flow_fw.shape == (npairs, h, w, 2), (frames.shape, flow_fw.shape)
    assert 1 <= weights.size <= TRAJ_MAX_RADIUS and ((weights >= 0) & (weights <= 1)).all(), weights
    assert tau >= np.finfo(_f32).tiny, tau
    out, support = np.empty_like(I), np.empty((npairs + 1, h, w), np.uint8)
    half = _f32(0.5)
    for f in range(npairs + 1):
        c = I[f].astype(_f32)
        wb, sb = _walk(I, c, f, False, flow_fw, flow_rev, weights, tau, fb_check, alpha, beta)
        wf, sf = _walk(I, c, f, True, flow_fw, flow_rev, weights, tau, fb_check, alpha, beta)
        num, den = c.copy(), np.ones((h, w), _f32)
        for j in range(weights.size):
            num = (num + wb[j][..., None] * sb[j]) + wf[j][..., None] * sf[j]
            den = (den + wb[j]) + wf[j]
        r = np.floor(num / den[..., None] + half)
        assert r.dtype == _f32
        out[f] = np.clip(r.astype(np.int64), 0, 255).astype(np.uint8)
        support[f] = (wf > 0).sum(axis=0).astype(np.uint8) | ((wb > 0).sum(axis=0).astype(np.uint8) << 4)
    return (out[..., 0] if gray else out), support
