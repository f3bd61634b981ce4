"""Numpy model of the point trajectories of include/ofdis.h (ofdis_track_points, ofdis_batch_track_points): the header's
definition operation by operation in float32, one rounding at a time.  Needs numpy only (no GPU, no library): the tests compare
the kernels against `track_ref` bit for bit, and a user can read a track array with `ended`.  Below it, the dense trajectories
(ofdis_seed_texture, ofdis_dense_tracks, ofdis_batch_dense_tracks): the grid, the integer texture test and the frame loop of
advance, occupancy and seeding (`dense_tracks_ref`), the selection of those tracks (ofdis_track_select): static, erratic, jumping
and camera-only tracks taken out and the rest compacted (`track_select_ref`, `TrackSelectParams`), and the descriptors of those tracks (ofdis_track_descriptors): HOG, HOF, MBH
and trajectory shape (`track_descriptors_ref`), where their channels lie (`descriptor_layout`) and their normalisation on the
host (`normalize_descriptors`).  Last, the bag-of-features encoding (ofdis_descriptor_normalize, ofdis_codebook_assign,
ofdis_bof_histogram, ofdis_track_bof): 8-bit RootSIFT descriptors, nearest words and their counts, integers throughout
(`normalize_descriptors_u8`, `codebook_assign_ref`, `bof_ref`), and the k-means training of its codebook (ofdis_codebook_seed,
ofdis_codebook_update, ofdis_codebook_train): evenly spread seeds and Lloyd's algorithm with integer means (`codebook_seed_ref`,
`codebook_update_ref`, `codebook_train_ref`).

    from of_dis_amd import tracking
    tracks, counts = batch.track_points(tracking.grid_seeds(w, h, 5), w, h)       # [n + 1][npoints][2], [npoints]
    alive = ~tracking.ended(tracks)                                              # [n + 1][npoints] bool
    T = tracking.min_eig_from_gradient(4.0, window=2, noc=1)                     # mean-tensor eigenvalue 4 -> the test's units
    dtracks, start, length, info = batch.dense_tracks(frames_ptr, w, h, 5, 2, T)  # [Lmax + 1][ntracks][2], step-major
    by_frame = tracking.to_frame_major(dtracks, start, length, n)                # [n + 1][ntracks][2], the layout above
    code, counts, dtracks, start, length, _, index, _ = capi.track_select(dtracks, start, length, models, (w, h))  # the kept ones
    hist, shape = capi.track_descriptors(frames, flow_fw, dtracks, start, length, 32, 2, 3, 0.4)   # [ntracks][396] u32
    desc = tracking.normalize_descriptors(hist, tracking.descriptor_layout(32, 2, 3), "rootsift")   # float64, per channel
    desc8 = capi.descriptor_normalize(hist, 2, 3)                                 # [ntracks][396] u8
    codebook = capi.codebook_train(desc8, capi.codebook_seed(desc8, 2, 3, 4000, length, 16), 2, 3, 10, length, 16)[0]
    bof = capi.track_bof(hist, length, codebook, 2, 3, min_len=16)                # [4][nwords] u32; codebook [nwords][396] u8
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


# ------------------------------------------------------------------ track selection (ofdis_track_select)
TS_KEPT, TS_SHORT, TS_INVALID, TS_STATIC, TS_ERRATIC, TS_JUMP, TS_CAMERA = range(7)  # include/ofdis.h: OFDIS_TS_*
TS_NAMES = ("kept", "short", "invalid", "static", "erratic", "jump", "camera")
TS_ALL_TESTS = 0x3F  # OFDIS_TS_ALL_TESTS


class TrackSelectParams:
    """include/ofdis.h: ofdis_track_select_params with the values of ofdis_track_select_defaults (Wang et al.'s)."""

    def __init__(self, min_len=0, min_std=1.7320508, max_std=50.0, max_step=20.0, max_step_share=0.7, min_camera=1.0,
                 tests=TS_ALL_TESTS):
        self.min_len, self.tests = int(min_len), int(tests)
        self.min_std, self.max_std, self.max_step = _f32(min_std), _f32(max_std), _f32(max_step)
        self.max_step_share, self.min_camera = _f32(max_step_share), _f32(min_camera)

    def __repr__(self):
        return (f"TrackSelectParams(min_len={self.min_len}, min_std={self.min_std!r}, max_std={self.max_std!r}, "
                f"max_step={self.max_step!r}, max_step_share={self.max_step_share!r}, min_camera={self.min_camera!r}, "
                f"tests={self.tests:#x})")


def _track_steps(tracks, start, models, size):
    """per step j < lmax: (d [n][2], r [n][2], has a model [n]) of the header's "step" and "residual step", float32"""
    lmax, n = tracks.shape[0] - 1, tracks.shape[1]
    if models is not None:
        models = np.asarray(models, np.float64)
        wide = models.ndim == 2 and models.shape[1] == 8   # the projective models of ofdis_track_select_projective
        models = models.reshape(-1, 8 if wide else 6)
        af = models.astype(_f32)
        cx, cy = _f32(size[0] - 1) * _f32(0.5), _f32(size[1] - 1) * _f32(0.5)
    for j in range(lmax):
        d = tracks[j + 1] - tracks[j]
        r, known = d, np.ones(n, bool)
        if models is not None:
            k = start + j
            known = (k >= 0) & (k < len(af))
            a = af[np.where(known, k, 0)]
            xc, yc = tracks[j, :, 0] - cx, tracks[j, :, 1] - cy
            mu = (a[:, 0] + a[:, 1] * xc) + a[:, 2] * yc
            mv = (a[:, 3] + a[:, 4] * xc) + a[:, 5] * yc
            if wide:
                pq = a[:, 6] * xc + a[:, 7] * yc
                mu, mv = mu + pq * xc, mv + pq * yc
            r = np.where(known[:, None], np.stack([d[:, 0] - mu, d[:, 1] - mv], 1), d)
        yield j, d, r, known


def track_select_ref(tracks, start, length, models=None, size=None, params=None, max_out=None):
    """The definition of ofdis_track_select in numpy float32, operation by operation.  tracks [lmax + 1][ntracks][2], start,
    length [ntracks] as dense_tracks_ref returns them; models float64 [npairs][6] as global_motion returns them (or [npairs][8]
    as projective_motion does: the definition of ofdis_track_select_projective) with size =
    (W, H) of their frames, or None; params a TrackSelectParams (None: the defaults); max_out the slots of the output set
    (None: room for every track) -> (code uint8 [ntracks], counts int64 [7], tracks_out [lmax + 1][nkept_written][2], start_out,
    len_out int32 [nkept_written], info_out int64 [2] = (nkept_written, dropped_out), index int32 [nkept_written], shape_out
    float32 [nkept_written][lmax][2])."""
    t = params if params is not None else TrackSelectParams()
    tracks = np.ascontiguousarray(tracks, _f32)
    start, length = np.asarray(start, np.int64), np.asarray(length, np.int64)
    lmax, n = tracks.shape[0] - 1, tracks.shape[1]
    assert lmax >= 1 and tracks.shape[2] == 2 and start.shape == length.shape == (n,), (tracks.shape, start.shape, length.shape)
    assert (models is None) or size is not None
    L = np.clip(length, 0, lmax + 1)
    fl = L.astype(_f32)
    with np.errstate(all="ignore"):
        finite = np.ones(n, bool)
        total = np.zeros((n, 2), _f32)
        for j in range(lmax + 1):
            on = L > j
            finite[on] &= np.isfinite(tracks[j, on]).all(1)
            total[on] = total[on] + tracks[j, on]
        mean = total / fl[:, None]
        var = np.zeros((n, 2), _f32)
        for j in range(lmax + 1):
            on = L > j
            e = tracks[j, on] - mean[on]
            var[on] = var[on] + e * e
        spread = np.sqrt(var / fl[:, None])
        S, Sr, mmax, rmax = (np.zeros(n, _f32) for _ in range(4))
        steps = []
        for j, d, r, known in _track_steps(tracks, start, models, size):
            on = L - 1 > j
            finite[on] &= known[on]
            m = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
            rm = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
            S[on], Sr[on] = S[on] + m[on], Sr[on] + rm[on]
            mmax[on] = np.where(m[on] > mmax[on], m[on], mmax[on])
            rmax[on] = np.where(rm[on] > rmax[on], rm[on], rmax[on])
            steps.append(r)
        sx, sy = spread[:, 0], spread[:, 1]
        holds = [None,
                 L < max(t.min_len, 1),
                 ~finite,
                 (sx < t.min_std) & (sy < t.min_std),
                 (sx > t.max_std) | (sy > t.max_std),
                 (L >= 2) & (mmax > t.max_step) & (mmax > S * t.max_step_share),
                 (L >= 2) & (rmax <= t.min_camera) if models is not None else np.zeros(n, bool)]
        code = np.zeros(n, np.uint8)
        for c in range(6, 0, -1):  # the first test that holds: the later ones are overwritten
            if (t.tests >> (c - 1)) & 1:
                code[holds[c]] = c
        counts = np.bincount(code, minlength=7).astype(np.int64)
        kept = np.flatnonzero(code == 0)
        room = len(kept) if max_out is None else int(max_out)
        index = kept[:room].astype(np.int32)
        shape = np.zeros((len(index), lmax, 2), _f32)
        for j, r in enumerate(steps):
            on = (L[index] - 1 > j) & (Sr[index] != 0)
            shape[on, j] = r[index[on]] / Sr[index[on], None]
    info = np.array([len(index), len(kept) - len(index)], np.int64)
    return (code, counts, np.ascontiguousarray(tracks[:, index]), start[index].astype(np.int32), length[index].astype(np.int32),
            info, index, shape)


# ------------------------------------------------------------------ trajectory-aligned descriptors (ofdis_track_descriptors)
DESC_MAX_PATCH = 64  # include/ofdis.h: OFDIS_DESC_MAX_PATCH
DESC_CHANNELS = (("hog", 8, 16.0), ("hof", 9, 256.0), ("mbhx", 8, 4096.0), ("mbhy", 8, 4096.0))  # name, bins, scale of quant
DESC_Q_MAX = 65535


def descriptor_layout(patch, nxy, nt):
    """Where the channels lie in a descriptor: {"dims": D = 33 * nxy^2 * nt, "cells": (nt, nxy, nxy), "channels": {name:
    (offset, bins)}} for "hog", "hof", "mbhx", "mbhy"; a channel is the block [offset, offset + bins * nt * nxy^2) of a hist row,
    shaped [nt][cell row][cell column][bin].  ValueError for the parameters ofdis_track_descriptor_dims answers with 0."""
    if not (2 <= patch <= DESC_MAX_PATCH and patch % 2 == 0 and 1 <= nxy <= 4 and patch % nxy == 0 and 1 <= nt <= 8):
        raise ValueError(f"patch {patch} (even, 2..{DESC_MAX_PATCH}), nxy {nxy} (1..4, dividing patch), nt {nt} (1..8)")
    cells = nt * nxy * nxy
    channels, at = {}, 0
    for name, bins, _ in DESC_CHANNELS:
        channels[name] = (at, bins)
        at += bins * cells
    return {"dims": at, "cells": (nt, nxy, nxy), "channels": channels}


def _octant(a, b):
    """oct(a, b) of include/ofdis.h by comparisons only: the bin 0..7, -1 where no case holds (zero vector, NaN)"""
    with np.errstate(invalid="ignore"):
        cases = [(a > 0) & (b >= 0), (a <= 0) & (b > 0), (a < 0) & (b <= 0), (a >= 0) & (b < 0)]
        pq = [(a, b), (b, -a), (-a, -b), (-b, a)]
        out = np.full(np.shape(a), -1, np.int64)
        for Q in (3, 2, 1, 0):  # (the first case that holds wins)
            p, q = pq[Q]
            out = np.where(cases[Q], 2 * Q + (q >= p), out)
    return out


def _quant(m, s):
    """quant(m, s) for finite float32 m: (values int64, clamped bool)"""
    with np.errstate(over="ignore"):
        ms = m * _f32(s)
    assert ms.dtype == _f32
    return np.floor(np.minimum(ms, _f32(DESC_Q_MAX)) + _f32(0.5)).astype(np.int64), ms > _f32(DESC_Q_MAX)


def _central(a):
    """(a[y][x+1] - a[y][x-1], a[y+1][x] - a[y-1][x]) with clamped neighbours"""
    h, w = a.shape
    xi, yi = np.arange(w), np.arange(h)
    with np.errstate(all="ignore"):
        return a[:, np.minimum(xi + 1, w - 1)] - a[:, np.maximum(xi - 1, 0)], a[np.minimum(yi + 1, h - 1)] - a[np.maximum(yi - 1, 0)]


def descriptor_features(frame, flow, min_flow):
    """frame uint8 [h][w] or [h][w][noc], flow float32 [h][w][2] -> per channel of DESC_CHANNELS (bin int64 [h][w], -1 where the
    pixel contributes nothing; q int64 [h][w]; clamped bool [h][w]): the votes of include/ofdis.h, one rounding at a time"""
    frame, flow = np.asarray(frame), np.asarray(flow, _f32)
    g = frame.astype(np.int64) if frame.ndim == 2 else frame.astype(np.int64).sum(-1)
    out = []
    gx, gy = _central(g)
    m = np.sqrt((gx * gx + gy * gy).astype(_f32))
    q, cl = _quant(m, 16.0)
    out.append((_octant(gx, gy), q, cl))
    u, v = flow[..., 0], flow[..., 1]
    with np.errstate(all="ignore"):
        m = np.sqrt(u * u + v * v)
        finite = np.isfinite(m)
        still = finite & (m < _f32(min_flow))
        q, cl = _quant(np.where(finite, m, _f32(0)), 256.0)
    out.append((np.where(still, 8, np.where(finite, _octant(u, v), -1)), np.where(still, 256, q), cl & finite & ~still))
    for c in (u, v):
        gx, gy = _central(c)
        with np.errstate(all="ignore"):
            m = np.sqrt(gx * gx + gy * gy)
            finite = np.isfinite(m)
            q, cl = _quant(np.where(finite, m, _f32(0)), 4096.0)
        assert m.dtype == _f32
        out.append((np.where(finite, _octant(gx, gy), -1), q, cl & finite))
    return out


def track_descriptors_ref(frames, flow_fw, tracks, start, length, patch, nxy, nt, min_flow, stats=None):
    """The definition of ofdis_track_descriptors in numpy.  frames uint8 [npairs + 1][h][w] (+ [noc]), flow_fw float32
    [npairs][h][w][2], tracks [lmax + 1][ntracks][2], start, length [ntracks] as dense_tracks_ref returns them -> (hist uint32
    [ntracks][D], shape float32 [ntracks][lmax][2]).  stats: an optional dict that receives "windows" (the windows visited: one
    per track and step), "cut" (those with a pixel outside the image), and over the window pixels inside the image and the four
    channels "clamped" (values quant clamped to 65535) and "skipped" (pixels that contribute nothing: no octant, not finite)."""
    frames, flow_fw = np.asarray(frames), np.asarray(flow_fw, _f32)
    tracks, start, length = np.asarray(tracks, _f32), np.asarray(start, np.int64), np.asarray(length, np.int64)
    npairs, h, w = flow_fw.shape[:3]
    lmax, n = tracks.shape[0] - 1, tracks.shape[1]
    layout = descriptor_layout(patch, nxy, nt)
    assert 1 <= nt <= lmax <= npairs and patch * patch * lmax <= 65536 and len(frames) == npairs + 1
    assert min_flow >= 0 and np.isfinite(min_flow)
    assert n == 0 or (length.min() >= 1 and length.max() <= lmax + 1 and start.min() >= 0 and (start + length - 1).max() <= npairs)
    D, cs = layout["dims"], patch // nxy
    hist = np.zeros(n * D, np.float64)  # (sums of integers below 2^32: exact)
    count = {"windows": 0, "cut": 0, "clamped": 0, "skipped": 0}
    feats = {}
    ab = np.arange(patch)
    b_, a_ = np.meshgrid(ab, ab, indexing="ij")  # window row b, column a
    cell = ((b_ // cs) * nxy + a_ // cs).ravel()
    a_, b_ = a_.ravel(), b_.ravel()
    for j in range(lmax):
        t = j * nt // lmax
        idx = np.flatnonzero(length - 1 > j)
        for k in np.unique(start[idx] + j):
            i = idx[start[idx] + j == k]
            if k not in feats:
                feats[k] = descriptor_features(frames[k], flow_fw[k], min_flow)
            cx = np.floor(tracks[j, i, 0] + _f32(0.5)).astype(np.int64)
            cy = np.floor(tracks[j, i, 1] + _f32(0.5)).astype(np.int64)
            x, y = cx[:, None] - patch // 2 + a_[None], cy[:, None] - patch // 2 + b_[None]
            ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
            count["windows"] += len(i)
            count["cut"] += int((~ok.all(1)).sum())
            x, y = x[ok], y[ok]
            row = np.broadcast_to(i[:, None] * D, ok.shape)[ok]  # the slot's row of hist
            tc = t * nxy * nxy + np.broadcast_to(cell[None], ok.shape)[ok]  # (t, cell row, cell column)
            for (name, bins, _), (bn, q, cl) in zip(DESC_CHANNELS, feats[k]):
                bv, qv = bn[y, x], q[y, x]
                votes = bv >= 0
                count["skipped"] += int((~votes).sum())
                count["clamped"] += int(cl[y, x].sum())
                at = row + layout["channels"][name][0] + tc * bins + bv
                hist += np.bincount(at[votes], weights=qv[votes], minlength=n * D)
    assert hist.max(initial=0) < 2 ** 32
    # the trajectory shape: the sequential float32 sum of the step lengths, then IEEE divisions
    shape = np.zeros((n, lmax, 2), _f32)
    S = np.zeros(n, _f32)
    with np.errstate(all="ignore"):
        d = tracks[1:] - tracks[:-1]  # [lmax][n][2]
        for j in range(lmax):
            on = length - 1 > j
            S[on] = S[on] + np.sqrt(d[j, on, 0] * d[j, on, 0] + d[j, on, 1] * d[j, on, 1])
        for j in range(lmax):
            on = (length - 1 > j) & (S != 0)
            shape[on, j] = d[j, on] / S[on, None]
    if stats is not None:
        stats.update(count)
    return hist.reshape(n, D).astype(np.uint32), shape


def normalize_descriptors(hist, layout, how="l2"):
    """hist [ntracks][D] (uint32 as the library writes it) -> float64 [ntracks][D], every channel of `layout`
    (descriptor_layout) normalised on its own: "l2": divided by its Euclidean norm; "rootsift": divided by its sum, then the
    square root (Arandjelovic and Zisserman 2012, as Wang et al. use it).  An all-zero channel stays zero."""
    if how not in ("l2", "rootsift"):
        raise ValueError(f"how = {how!r}: 'l2' or 'rootsift'")
    hist = np.asarray(hist)
    assert hist.ndim == 2 and hist.shape[1] == layout["dims"], (hist.shape, layout["dims"])
    out = hist.astype(np.float64)
    cells = int(np.prod(layout["cells"]))
    for off, bins in layout["channels"].values():
        v = out[:, off:off + bins * cells]
        norm = np.sqrt((v * v).sum(1)) if how == "l2" else v.sum(1)
        v /= np.where(norm > 0, norm, 1.0)[:, None]
        if how == "rootsift":
            np.sqrt(v, out=v)
    return out


# ------------------------------------------------------------------ bag of features (ofdis_descriptor_normalize .. ofdis_track_bof)
BOF_SCALE, BOF_MAX_WORDS = 510, 16384  # include/ofdis.h: OFDIS_BOF_*


def _channel_slices(layout):
    """the four channels of a row in the order HOG, HOF, MBHx, MBHy"""
    cells = int(np.prod(layout["cells"]))
    return [slice(off, off + bins * cells) for off, bins in (layout["channels"][name] for name, _, _ in DESC_CHANNELS)]


def normalize_descriptors_u8(hist, layout):
    """The definition of ofdis_descriptor_normalize in numpy, division-free as the header states it: hist uint32 [ntracks][D] ->
    uint8 [ntracks][D], per channel of `layout` (descriptor_layout) with its uint64 sum S: desc = min(255, max{q >= 0 :
    q * q * S <= 510 * 510 * h}), all zero where S == 0.  Every product is an exact uint64 below 2^62; float64 only proposes a q
    that the exact comparisons then move."""
    hist = np.asarray(hist)
    assert hist.dtype == np.uint32 and hist.ndim == 2 and hist.shape[1] == layout["dims"], (hist.dtype, hist.shape, layout["dims"])
    out = np.zeros(hist.shape, np.uint8)
    one = np.uint64(1)
    for seg in _channel_slices(layout):
        h = hist[:, seg].astype(np.uint64)
        S = np.broadcast_to(h.sum(1, dtype=np.uint64)[:, None], h.shape)
        T = h * np.uint64(BOF_SCALE * BOF_SCALE)
        q = np.floor(np.sqrt(T.astype(np.float64) / np.maximum(S, one).astype(np.float64))).astype(np.uint64)
        while True:  # down while q q S > T, then up while (q + 1)^2 S <= T (q <= 510: h <= S)
            high = (q * q * S > T) & (q > 0)
            if not high.any():
                break
            q[high] -= one
        while True:
            low = ((q + one) * (q + one) * S <= T) & (S > 0)
            if not low.any():
                break
            q[low] += one
        out[:, seg] = np.minimum(np.where(S > 0, q, 0), 255).astype(np.uint8)
    return out


def codebook_assign_ref(desc, layout, codebook):
    """The definition of ofdis_codebook_assign in numpy, by direct differences in int64: desc uint8 [ntracks][D], codebook uint8
    [nwords][D] -> (words, dist), each int32 [ntracks][4]: per channel the lowest index of the nearest word (np.argmin returns the
    first minimum) and its squared distance."""
    desc, codebook = np.asarray(desc), np.asarray(codebook)
    assert desc.dtype == codebook.dtype == np.uint8 and desc.ndim == codebook.ndim == 2, (desc.dtype, codebook.dtype)
    assert desc.shape[1] == codebook.shape[1] == layout["dims"] and 1 <= len(codebook) <= BOF_MAX_WORDS, (desc.shape, codebook.shape)
    n = len(desc)
    words, dist = np.zeros((n, 4), np.int32), np.zeros((n, 4), np.int32)
    for c, seg in enumerate(_channel_slices(layout)):
        x, cb = desc[:, seg].astype(np.int64), codebook[:, seg].astype(np.int64)
        step = max(1, (1 << 22) // max(1, cb.size))  # tracks at a time: about 32 MB of differences
        for i in range(0, n, step):
            diff = x[i:i + step, None, :] - cb[None]
            d = (diff * diff).sum(-1)
            k = d.argmin(1)
            words[i:i + step, c], dist[i:i + step, c] = k, d[np.arange(len(k)), k]
    return words, dist


def bof_ref(words, length, nwords, min_len=1):
    """The definition of ofdis_bof_histogram in numpy: words int [ntracks][4], length [ntracks] -> uint32 [4][nwords], row c the
    count of every word of channel c over the tracks with length >= min_len; a word outside 0 .. nwords - 1 is not counted."""
    words, length = np.asarray(words, np.int64), np.asarray(length, np.int64)
    assert words.ndim == 2 and words.shape[1] == 4 and length.shape == (len(words),) and min_len >= 1 and nwords >= 1
    w = words[length >= min_len]
    return np.stack([np.bincount(col[(col >= 0) & (col < nwords)], minlength=nwords) for col in w.T]).astype(np.uint32)


# ------------------------------------------------------------------ codebook training (ofdis_codebook_seed .. ofdis_codebook_train)
KMEANS_MAX_ITERS = 1000  # include/ofdis.h: OFDIS_KMEANS_MAX_ITERS


def _members(length, n, min_len):
    """bool [n]: the slots that train -- all of them without a length array, else the tracks of at least min_len points"""
    assert min_len >= 1
    if length is None:
        return np.ones(n, bool)
    length = np.asarray(length)
    assert length.shape == (n,), (length.shape, n)
    return length >= min_len


def codebook_seed_ref(desc, length, nwords, min_len=1):
    """The definition of ofdis_codebook_seed in numpy: desc uint8 [ntracks][D], length [ntracks] or None -> uint8 [nwords][D]: row
    k is the desc row of the first member at or after slot s_k = floor((2 k + 1) ntracks / (2 nwords)), cyclically; all zero
    where there is no member."""
    desc = np.asarray(desc)
    assert desc.dtype == np.uint8 and desc.ndim == 2 and 1 <= nwords <= BOF_MAX_WORDS, (desc.dtype, desc.shape, nwords)
    n = len(desc)
    out = np.zeros((nwords, desc.shape[1]), np.uint8)
    at = np.flatnonzero(_members(length, n, min_len))
    if len(at):
        for k in range(nwords):
            s = (2 * k + 1) * n // (2 * nwords)
            j = np.searchsorted(at, s)              # the first member >= s_k, else the first one of all
            out[k] = desc[at[j] if j < len(at) else at[0]]
    return out


def codebook_update_ref(desc, layout, words, length, codebook, min_len=1):
    """The definition of ofdis_codebook_update in numpy: desc uint8 [ntracks][D], words int [ntracks][4], length [ntracks] or
    None, codebook uint8 [nwords][D] -> (codebook, counts uint32 [4][nwords]).  Per channel, a word with members M becomes
    floor((2 S + |M|) / (2 |M|)) of their int64 sums S, the mean rounded half up; a word without members keeps its bytes; a
    words entry outside 0 .. nwords - 1 belongs to no word."""
    desc, codebook, words = np.asarray(desc), np.asarray(codebook), np.asarray(words, np.int64)
    assert desc.dtype == codebook.dtype == np.uint8 and desc.shape[1] == codebook.shape[1] == layout["dims"], (desc.shape, codebook.shape)
    n, nwords = len(desc), len(codebook)
    assert words.shape == (n, 4) and 1 <= nwords <= BOF_MAX_WORDS, (words.shape, nwords)
    member = _members(length, n, min_len)
    out, counts = codebook.copy(), np.zeros((4, nwords), np.uint32)
    for c, seg in enumerate(_channel_slices(layout)):
        w = words[:, c]
        use = member & (w >= 0) & (w < nwords)
        cnt = np.bincount(w[use], minlength=nwords).astype(np.int64)
        S = np.zeros((nwords, seg.stop - seg.start), np.int64)
        np.add.at(S, w[use], desc[use, seg].astype(np.int64))
        has = cnt > 0
        out[has, seg] = ((2 * S[has] + cnt[has, None]) // (2 * cnt[has, None])).astype(np.uint8)
        counts[c] = cnt
    return out, counts


def codebook_train_ref(desc, layout, length, codebook, iters, min_len=1):
    """The definition of ofdis_codebook_train in numpy: iters rounds of codebook_assign_ref + codebook_update_ref from `codebook`
    -> (codebook, words int32 [ntracks][4], counts uint32 [4][nwords], stats int64 [iters][4][2]); stats[t][c] = (the members
    whose word differs from round t - 1, all members at t = 0; the sum of the members' squared distances).  words and counts are
    those of the last assignment, taken against the codebook before the last update."""
    assert 1 <= iters <= KMEANS_MAX_ITERS, iters
    codebook = np.asarray(codebook).copy()
    member = _members(length, len(desc), min_len)
    stats = np.zeros((iters, 4, 2), np.int64)
    words = counts = None
    for t in range(iters):
        before = words
        words, dist = codebook_assign_ref(desc, layout, codebook)
        changed = np.ones(words.shape, bool) if before is None else words != before
        stats[t, :, 0] = (changed & member[:, None]).sum(0)
        stats[t, :, 1] = dist[member].astype(np.int64).sum(0)
        codebook, counts = codebook_update_ref(desc, layout, words, length, codebook, min_len)
    return codebook, words, counts, stats
