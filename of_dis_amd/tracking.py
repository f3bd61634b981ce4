"""Numpy model of the point trajectories of include/ofdis.h (ofdis_track_points, ofdis_batch_track_points): the header's
definition operation by operation in float32, one rounding at a time.  Needs numpy only (no GPU, no library): the tests compare
the kernels against `track_ref` bit for bit, and a user can read a track array with `ended`.

    from of_dis_amd import tracking
    tracks, counts = batch.track_points(tracking.grid_seeds(w, h, 5), w, h)       # [n + 1][npoints][2], [npoints]
    alive = ~tracking.ended(tracks)                                              # [n + 1][npoints] bool
"""
import numpy as np

FB_ALPHA, FB_BETA = 0.01, 0.5  # include/ofdis.h: OFDIS_FB_ALPHA / OFDIS_FB_BETA (capi.FB_ALPHA / FB_BETA)
ENDED_BITS = 0x7FC00000  # both components of an entry that belongs to no track

_f32 = np.float32


def ended(tracks):
    """[..., 2] float32 track entries -> bool [...]: True where the entry belongs to no track (a track never holds a NaN)."""
    return np.isnan(np.asarray(tracks)[..., 0])


def grid_seeds(width, height, stride):
    """The integer grid (0, stride, 2 * stride, ...)^2 inside a width x height frame, row by row: [npoints][2] float32 (x, y)."""
    ys, xs = np.meshgrid(np.arange(0, height, stride), np.arange(0, width, stride), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel()], axis=1).astype(_f32)


def inside(px, py, w, h):
    """0 <= px <= w-1 and 0 <= py <= h-1 (NaN: False)"""
    with np.errstate(invalid="ignore"):
        return (px >= _f32(0)) & (px <= _f32(w - 1)) & (py >= _f32(0)) & (py <= _f32(h - 1))


def bilinear(F, px, py):
    """F [h][w][2] float32 sampled at the positions (px, py) INSIDE the image: (u, v), each float32 [n]"""
    h, w, _ = F.shape
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
    with np.errstate(all="ignore"):
        r = (F[y0, x0] * bx + F[y0, x1] * ax) * by + (F[y1, x0] * bx + F[y1, x1] * ax) * ay
    assert r.dtype == _f32
    return r[:, 0], r[:, 1]


def consistent(u, v, ru, rv, alpha, beta):
    """the forward-backward inequality of ofdis_fb_check (a NaN on either side: False)"""
    with np.errstate(all="ignore"):
        du, dv = u + ru, v + rv
        lhs = du * du + dv * dv
        rhs = _f32(alpha) * ((u * u + v * v) + (ru * ru + rv * rv)) + _f32(beta)
        return lhs <= rhs


def track_ref(flow_fw, flow_rev, seeds, seed_frame=None, max_steps=0, alpha=FB_ALPHA, beta=FB_BETA, reasons=None):
    """flow_fw [npairs][h][w][2] float32, flow_rev the same or None, seeds [npoints][2], seed_frame [npoints] int or None ->
    (tracks [npairs + 1][npoints][2] float32, counts [npoints] int32), the arrays ofdis_track_points writes.
    reasons: an optional dict that receives how many tracks ended by leaving the image ("outside") and by the inequality
    ("inconsistent")."""
    flow_fw = np.asarray(flow_fw, _f32)
    flow_rev = None if flow_rev is None else np.asarray(flow_rev, _f32)
    seeds = np.asarray(seeds, _f32)
    npairs, h, w = flow_fw.shape[:3]
    n = seeds.shape[0]
    s = np.zeros(n, np.int64) if seed_frame is None else np.asarray(seed_frame, np.int64)
    tracks = np.full((npairs + 1, n, 2), ENDED_BITS, np.uint32).view(_f32)
    counts = np.zeros(n, np.int32)
    px, py = seeds[:, 0].copy(), seeds[:, 1].copy()
    seeded = (s >= 0) & (s <= npairs) & inside(px, py, w, h)
    live = np.zeros(n, bool)
    ends = {"outside": 0, "inconsistent": 0}
    for f in range(npairs + 1):
        live |= seeded & (s == f)
        tracks[f, live, 0], tracks[f, live, 1] = px[live], py[live]
        counts[live] += 1
        live &= (f < npairs) & ((max_steps == 0) | (f - s < max_steps))
        i = np.flatnonzero(live)
        if i.size == 0:
            continue
        u, v = bilinear(flow_fw[f], px[i], py[i])
        with np.errstate(all="ignore"):
            qx, qy = px[i] + u, py[i] + v
        ok = inside(qx, qy, w, h)
        ends["outside"] += int((~ok).sum())
        if flow_rev is not None:
            j = np.flatnonzero(ok)
            ru, rv = bilinear(flow_rev[f], qx[j], qy[j])
            c = consistent(u[j], v[j], ru, rv, alpha, beta)
            ends["inconsistent"] += int((~c).sum())
            ok[j] = c
        px[i], py[i] = qx, qy
        live[i] = ok
    if reasons is not None:
        reasons.update(ends)
    return tracks, counts
