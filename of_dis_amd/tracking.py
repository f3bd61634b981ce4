"""Numpy model of the point trajectories of include/ofdis.h (ofdis_track_points, ofdis_batch_track_points): the header's
definition operation by operation in float32, one rounding at a time.  Needs numpy only (no GPU, no library): the tests compare
the kernels against `track_ref` bit for bit, and a user can read a track array with `ended`.  Below it, the dense trajectories
(ofdis_seed_texture, ofdis_dense_tracks, ofdis_batch_dense_tracks): the grid, the integer texture test and the frame loop of
advance, occupancy and seeding (`dense_tracks_ref`).

    from of_dis_amd import tracking
    tracks, counts = batch.track_points(tracking.grid_seeds(w, h, 5), w, h)       # [n + 1][npoints][2], [npoints]
    alive = ~tracking.ended(tracks)                                              # [n + 1][npoints] bool
    T = tracking.min_eig_from_gradient(4.0, window=2, noc=1)                     # mean-tensor eigenvalue 4 -> the test's units
    dtracks, start, length, info = batch.dense_tracks(frames_ptr, w, h, 5, 2, T)  # [Lmax + 1][ntracks][2], step-major
    by_frame = tracking.to_frame_major(dtracks, start, length, n)                # [n + 1][ntracks][2], the layout above
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


# ------------------------------------------------------------------ dense trajectories (ofdis_seed_texture, ofdis_dense_tracks)
DT_MAX_TRACKS, DT_MAX_STRIDE, DT_MAX_WINDOW = 1 << 24, 64, 7  # include/ofdis.h: OFDIS_DT_MAX_*


def dense_grid(width, height, stride):
    """(ncx, ncy): the cells of the seed grid of a width x height frame.  Cell (cx, cy) has the centre pixel
    (stride // 2 + cx * stride, stride // 2 + cy * stride); cells are numbered row by row."""
    off = stride // 2
    return (width - 1 - off) // stride + 1, (height - 1 - off) // stride + 1


def dense_centres(width, height, stride):
    """(xs [ncx], ys [ncy]) int64: the centre pixels of the grid's columns and rows"""
    ncx, ncy = dense_grid(width, height, stride)
    return stride // 2 + stride * np.arange(ncx), stride // 2 + stride * np.arange(ncy)


def dense_cell(px, py, width, height, stride):
    """the cell number of positions inside the image"""
    ncx, ncy = dense_grid(width, height, stride)
    cx = np.minimum(np.floor(px).astype(np.int64) // stride, ncx - 1)
    cy = np.minimum(np.floor(py).astype(np.int64) // stride, ncy - 1)
    return cy * ncx + cx


def structure_tensor(frames, stride, window):
    """frames uint8 [n][h][w] or [n][h][w][noc] -> (a, b, c), each int64 [n][ncy][ncx]: the sums of gx*gx, gx*gy and gy*gy of
    the header's definition over the window of every cell centre and the channels"""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim in (3, 4), (frames.dtype, frames.shape)
    I = (frames if frames.ndim == 4 else frames[..., None]).astype(np.int64)
    n, h, w, _ = I.shape
    xi, yi = np.arange(w), np.arange(h)
    gx = I[:, :, np.minimum(xi + 1, w - 1)] - I[:, :, np.maximum(xi - 1, 0)]
    gy = I[:, np.minimum(yi + 1, h - 1)] - I[:, np.maximum(yi - 1, 0)]
    A, B, Cc = (gx * gx).sum(-1), (gx * gy).sum(-1), (gy * gy).sum(-1)
    xs, ys = dense_centres(w, h, stride)
    a, b, c = (np.zeros((n, len(ys), len(xs)), np.int64) for _ in range(3))
    for j in range(-window, window + 1):
        yy = np.clip(ys + j, 0, h - 1)
        for i in range(-window, window + 1):
            xx = np.clip(xs + i, 0, w - 1)
            a += A[:, yy][:, :, xx]
            b += B[:, yy][:, :, xx]
            c += Cc[:, yy][:, :, xx]
    return a, b, c


def seed_texture_ref(frames, stride, window, min_eig):
    """frames uint8 [n][h][w] or [n][h][w][noc] -> uint8 [n][ncy][ncx], 1 where the smaller eigenvalue of the structure tensor
    at the cell centre is >= min_eig (exact integer arithmetic), what ofdis_seed_texture writes"""
    a, b, c = structure_tensor(frames, stride, window)
    T = int(min_eig)
    return ((a >= T) & (c >= T) & ((a - T) * (c - T) >= b * b)).astype(np.uint8)


def min_eig_from_gradient(lam, window, noc):
    """The threshold min_eig that stands for the eigenvalue `lam` of the MEAN structure tensor of true central differences
    (grey levels per pixel, squared): the library sums doubled differences over (2 * window + 1)^2 pixels and noc channels."""
    return int(min(max(np.ceil(float(lam) * 4 * (2 * window + 1) ** 2 * noc), 0), 2 ** 31 - 1))


def dense_tracks_ref(frames, flow_fw, flow_rev, stride, window, min_eig, max_len=15, max_tracks=None, alpha=FB_ALPHA,
                     beta=FB_BETA, reasons=None):
    """frames uint8 [npairs + 1][h][w] (+ [noc]), flow_fw [npairs][h][w][2] float32, flow_rev the same or None -> (tracks
    [Lmax + 1][ntracks][2] float32, start [ntracks] int32, len [ntracks] int32, info int64 [2] = (ntracks, dropped)): the slots
    below ntracks of what ofdis_dense_tracks writes (the library's arrays have max_tracks slots per step).  max_tracks None:
    room for every seed.  reasons: an optional dict that receives how many tracks ended by leaving the image ("outside"), by
    the inequality ("inconsistent") and by reaching Lmax + 1 frames ("complete"), how many started after frame 0 ("reseeds")
    and how many seeds found no slot ("dropped")."""
    flow_fw = np.asarray(flow_fw, _f32)
    flow_rev = None if flow_rev is None else np.asarray(flow_rev, _f32)
    npairs, h, w = flow_fw.shape[:3]
    assert len(frames) == npairs + 1, (len(frames), npairs)
    ncx, ncy = dense_grid(w, h, stride)
    ncells = ncx * ncy
    lmax = min(max_len, npairs) if max_len else npairs
    room = npairs * ncells
    max_tracks = room if max_tracks is None else int(max_tracks)
    cap = min(room, max_tracks)
    tex = seed_texture_ref(np.asarray(frames)[:npairs], stride, window, min_eig).reshape(npairs, ncells).astype(bool)
    xs, ys = dense_centres(w, h, stride)
    centre_x, centre_y = np.tile(xs, ncy).astype(_f32), np.repeat(ys, ncx).astype(_f32)
    tracks = np.full((lmax + 1, cap, 2), ENDED_BITS, np.uint32).view(_f32)
    start, length = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    px, py, live = np.zeros(cap, _f32), np.zeros(cap, _f32), np.zeros(cap, bool)
    n = dropped = 0
    why = {"outside": 0, "inconsistent": 0, "complete": 0, "reseeds": 0, "dropped": 0}
    for f in range(npairs + 1):
        i = np.flatnonzero(live)
        if f >= 1 and i.size:
            u, v = bilinear(flow_fw[f - 1], px[i], py[i])
            with np.errstate(all="ignore"):
                qx, qy = px[i] + u, py[i] + v
            ok = inside(qx, qy, w, h)
            why["outside"] += int((~ok).sum())
            if flow_rev is not None:
                j = np.flatnonzero(ok)
                ru, rv = bilinear(flow_rev[f - 1], qx[j], qy[j])
                c = consistent(u[j], v[j], ru, rv, alpha, beta)
                why["inconsistent"] += int((~c).sum())
                ok[j] = c
            i, qx, qy = i[ok], qx[ok], qy[ok]
            live[:] = False
            tracks[length[i], i, 0], tracks[length[i], i, 1] = qx, qy
            px[i], py[i] = qx, qy
            length[i] += 1
            done = length[i] == lmax + 1
            why["complete"] += int(done.sum())
            live[i[~done]] = True
        if f == npairs:
            break
        occupied = np.zeros(ncells, bool)
        k = np.flatnonzero(live)
        occupied[dense_cell(px[k], py[k], w, h, stride)] = True
        cells = np.flatnonzero(~occupied & tex[f])
        take = cells[:max_tracks - n]
        dropped += len(cells) - len(take)
        s = slice(n, n + len(take))
        px[s], py[s] = centre_x[take], centre_y[take]
        tracks[0, s, 0], tracks[0, s, 1] = px[s], py[s]
        start[s], length[s], live[s] = f, 1, True
        why["reseeds"] += len(take) if f else 0
        n += len(take)
    why["dropped"] = dropped
    if reasons is not None:
        reasons.update(why)
    return np.ascontiguousarray(tracks[:, :n]), start[:n].copy(), length[:n].copy(), np.array([n, dropped], np.int64)


def to_frame_major(tracks, start, length, npairs):
    """the step-major arrays of dense_tracks -> [npairs + 1][ntracks][2] float32 in the layout of ofdis_track_points:
    entry [f][i] is track i in frame f, the 0x7FC00000 NaN where it does not exist"""
    tracks, start, length = np.asarray(tracks, _f32), np.asarray(start), np.asarray(length)
    n = start.shape[0]
    out = np.full((npairs + 1, n, 2), ENDED_BITS, np.uint32).view(_f32)
    for j in range(tracks.shape[0]):
        i = np.flatnonzero(length > j)
        out[start[i] + j, i] = tracks[j, i]
    return out
