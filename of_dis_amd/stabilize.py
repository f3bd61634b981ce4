"""Numpy model of the video stabilisation of include/ofdis.h (ofdis_camera_path, ofdis_warp_frames and ofdis_batch_stabilize):
the header's definition in its order -- the camera path in float64 and the frame warp in float32, one rounding per operation.
Needs numpy only (no GPU, no library): the tests compare the kernels against `camera_path_ref` and `warp_frames_ref` bit for
bit.

    from of_dis_amd import stabilize
    weights = stabilize.gaussian_weights(radius=8, sigma=4.0)
    warps = stabilize.camera_path_ref(models, weights, zoom=1.1)            # models: ofdis_global_motion's, [npairs][6]
    out, inside = stabilize.warp_frames_ref(frames, warps, stabilize.BORDER_REPLICATE)

The projective twins (ofdis_camera_path_projective, ofdis_warp_frames_projective) take the 8-parameter models of
ofdis_projective_motion: the path is chained, averaged and inverted on homographies, the frames are resampled by a perspective
warp.  The affine functions above them are untouched.

    warps8 = stabilize.camera_path_projective_ref(models8, weights, 1.1, w, h)   # models8: [npairs][8] -> warps [npairs + 1][8]
    out, inside = stabilize.warp_frames_projective_ref(frames, warps8)
"""
import math

import numpy as np

from .temporal import inside as _inside, sample as _sample

STAB_MAX_RADIUS = 64                        # include/ofdis.h: OFDIS_STAB_MAX_RADIUS
STAB_MIN_DET, STAB_MAX_DET = 0.25, 4.0      # OFDIS_STAB_MIN_DET / OFDIS_STAB_MAX_DET
STAB_MAX_ZOOM = 16.0                        # OFDIS_STAB_MAX_ZOOM
STAB_MIN_DENOM = 0.5                        # include/ofdis.h, "Projective video stabilisation": the denominator bound of usable()
BORDER_CONSTANT, BORDER_REPLICATE = 0, 1    # OFDIS_BORDER_*
GM_MAX_SIDE = 8192                          # OFDIS_GM_MAX_SIDE

_f32 = np.float32
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)   # a map (a, b, c, d, tx, ty): x' = a*x + b*y + tx, y' = c*x + d*y + ty


def gaussian_weights(radius, sigma):
    """the window exp(-j^2 / (2 sigma^2)), j = 0 .. radius, as float64 [radius + 1] (w_0 = 1)"""
    if not 0 <= radius <= STAB_MAX_RADIUS:
        raise ValueError("radius outside 0..STAB_MAX_RADIUS")
    if not (math.isfinite(sigma) and sigma > 0):
        raise ValueError("sigma must be finite and > 0")
    j = np.arange(radius + 1, dtype=np.float64)
    return np.exp(-(j * j) / (2.0 * float(sigma) * float(sigma)))


def check_window(weights, zoom):
    """the weights as float64 [radius + 1], checked as ofdis_camera_path checks them; raises ValueError"""
    weights = np.ascontiguousarray(weights, np.float64)
    if weights.ndim != 1 or not 1 <= weights.size <= STAB_MAX_RADIUS + 1:
        raise ValueError("weights: radius + 1 values, radius in 0..STAB_MAX_RADIUS")
    if not (np.isfinite(weights).all() and weights[0] > 0 and (weights >= 0).all()):
        raise ValueError("weights must be finite, w_0 > 0 and the others >= 0")
    if not (math.isfinite(zoom) and 1.0 <= zoom <= STAB_MAX_ZOOM):
        raise ValueError("zoom must be inside [1, STAB_MAX_ZOOM]")
    return weights


def det_ok(det):
    """STAB_MIN_DET <= det <= STAB_MAX_DET (NaN: False)"""
    return det >= STAB_MIN_DET and det <= STAB_MAX_DET


def pair_map(a):
    """T_k of a model a [6]: (map, usable).  Python floats are IEEE doubles and every operation is rounded on its own."""
    a = [float(v) for v in a]
    if not all(math.isfinite(v) for v in a):
        return None, False
    T = (1.0 + a[1], a[2], a[4], 1.0 + a[5], a[0], a[3])
    return T, det_ok(T[0] * T[3] - T[1] * T[2])


def compose(T, M):
    """T o M: M first, then T"""
    return (T[0] * M[0] + T[1] * M[2], T[0] * M[1] + T[1] * M[3], T[2] * M[0] + T[3] * M[2], T[2] * M[1] + T[3] * M[3],
            (T[0] * M[4] + T[1] * M[5]) + T[4], (T[2] * M[4] + T[3] * M[5]) + T[5])


def invert(T, det):
    """the inverse of T, det = T.a*T.d - T.b*T.c computed by the caller (0 - x: a zero entry stays +0)"""
    ia, ib, ic, id_ = T[3] / det, (0.0 - T[1]) / det, (0.0 - T[2]) / det, T[0] / det
    return (ia, ib, ic, id_, 0.0 - (ia * T[4] + ib * T[5]), 0.0 - (ic * T[4] + id_ * T[5]))


def smoothed_map(models, f, weights):
    """Q_f and the reach r_f of frame f: the window walked outwards from f, stopped at the first unusable pair on either side"""
    npairs = len(models)
    w0 = float(weights[0])
    acc = [w0, 0.0, 0.0, w0, 0.0, 0.0]
    sw = w0
    Mf = Mb = IDENTITY
    r = 0
    for j in range(1, len(weights)):
        if f + j - 1 >= npairs or f - j < 0:
            break
        Tf, okf = pair_map(models[f + j - 1])
        Tb, okb = pair_map(models[f - j])
        if not (okf and okb):
            break
        Mf = compose(Tf, Mf)
        Mb = compose(invert(Tb, Tb[0] * Tb[3] - Tb[1] * Tb[2]), Mb)
        wj = float(weights[j])
        acc = [acc[e] + (wj * Mf[e] + wj * Mb[e]) for e in range(6)]
        sw = sw + (wj + wj)
        r = j
    return tuple(v / sw for v in acc), r   # (sw >= w_0 > 0)


def correction(Q, zoom):
    """the warp of a frame from its smoothed map: W = Q^-1 (the identity where det Q is outside the limits or W is not finite),
    zoomed about the centre, in the displacement parametrisation b [6]"""
    det = Q[0] * Q[3] - Q[1] * Q[2]
    W = IDENTITY
    if det_ok(det):
        W = invert(Q, det)
        if not all(math.isfinite(v) for v in W):
            W = IDENTITY
    s = 1.0 / float(zoom)
    return (W[4], W[0] * s - 1.0, W[1] * s, W[5], W[2] * s, W[3] * s - 1.0)


def camera_path_ref(models, weights, zoom=1.0):
    """models [npairs][6] float64 (ofdis_global_motion's parametrisation), weights [radius + 1] float64 -> warps
    [npairs + 1][6] float64, what ofdis_camera_path writes"""
    weights = check_window(weights, zoom)
    models = np.ascontiguousarray(models, np.float64)
    assert models.ndim == 2 and models.shape[1] == 6 and models.shape[0] >= 1, models.shape
    warps = np.empty((models.shape[0] + 1, 6), np.float64)
    for f in range(models.shape[0] + 1):
        warps[f] = correction(smoothed_map(models, f, weights)[0], zoom)
    return warps


def warp_positions(b, w, h):
    """the sample positions of a warp b [6] (float64, converted to float32 first): (px, py), float32 [h][w] each"""
    X = (2 * np.arange(w, dtype=np.int64) - (w - 1))[None, :]
    Y = (2 * np.arange(h, dtype=np.int64) - (h - 1))[:, None]
    with np.errstate(all="ignore"):
        bf = np.asarray(b, np.float64).astype(_f32)
        xc, yc = X.astype(_f32) * _f32(0.5), Y.astype(_f32) * _f32(0.5)
        mu = (bf[0] + bf[1] * xc) + bf[2] * yc
        mv = (bf[3] + bf[4] * xc) + bf[5] * yc
        px = np.arange(w, dtype=np.int64).astype(_f32)[None, :] + mu
        py = np.arange(h, dtype=np.int64).astype(_f32)[:, None] + mv
    assert px.dtype == _f32 and py.dtype == _f32 and px.shape == py.shape == (h, w)
    return px, py


def warp_frames_ref(frames, warps, border=BORDER_CONSTANT):
    """frames [n][h][w] (gray) or [n][h][w][3] uint8, warps [n][6] float64 -> (out, the shape of frames, uint8; inside
    [n][h][w] uint8), the arrays ofdis_warp_frames writes"""
    if border not in (BORDER_CONSTANT, BORDER_REPLICATE):
        raise ValueError("border must be BORDER_CONSTANT or BORDER_REPLICATE")
    frames = np.asarray(frames, np.uint8)
    gray = frames.ndim == 3
    I = frames[..., None] if gray else frames
    n, h, w, noc = I.shape
    assert noc in (1, 3) and max(w, h) <= GM_MAX_SIDE, frames.shape
    warps = np.asarray(warps, np.float64).reshape(n, 6)
    out, ins_out = np.empty_like(I), np.empty((n, h, w), np.uint8)
    for f in range(n):
        px, py = warp_positions(warps[f], w, h)
        ins = _inside(px, py, w, h)
        # (fmax / fmin return the other operand for a NaN, like fmaxf / fminf: a NaN position samples pixel 0)
        pxc = np.fmin(np.fmax(px, _f32(0)), _f32(w - 1))
        pyc = np.fmin(np.fmax(py, _f32(0)), _f32(h - 1))
        c = _sample(I[f], pxc.ravel(), pyc.ravel()).reshape(h, w, noc)
        if border == BORDER_CONSTANT:
            c = np.where(ins[..., None], c, _f32(0))
        r = np.floor(c + _f32(0.5))
        assert r.dtype == _f32
        out[f] = np.clip(r.astype(np.int64), 0, 255).astype(np.uint8)
        ins_out[f] = ins
    return (out[..., 0] if gray else out), ins_out


# ------------------------------------------------------------------ the projective path and warp (include/ofdis.h: "Projective
# video stabilisation").  A map is (a, b, c, d, tx, ty, gx, gy) with an implicit 1 in the corner of the 3 x 3 matrix:
# x' = (a*x + b*y + tx) / (1 + gx*x + gy*y), y' = (c*x + d*y + ty) / (1 + gx*x + gy*y)
IDENTITY8 = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0)


def half_sides(w, h):
    """(hx, hy) = ((W-1)/2, (H-1)/2) of a frame, checked as ofdis_camera_path_projective checks its sides; raises ValueError"""
    if not (1 <= w <= GM_MAX_SIDE and 1 <= h <= GM_MAX_SIDE):
        raise ValueError("sides outside 1..GM_MAX_SIDE")
    return (w - 1) / 2.0, (h - 1) / 2.0


def usable8(T, hx, hy):
    """all eight numbers finite, the determinant of the linear part inside its limits and the denominator at least
    STAB_MIN_DENOM over the whole frame (a NaN fails every comparison)"""
    if not all(math.isfinite(v) for v in T):
        return False
    return det_ok(T[0] * T[3] - T[1] * T[2]) and (1.0 - abs(T[6]) * hx) - abs(T[7]) * hy >= STAB_MIN_DENOM


def pair_map8(a, hx, hy):
    """T_k of a model a [8]: (map, usable)"""
    a = [float(v) for v in a]
    if not all(math.isfinite(v) for v in a):
        return None, False
    T = (1.0 + a[1], a[2], a[4], 1.0 + a[5], a[0], a[3], 0.0 - a[6], 0.0 - a[7])
    return T, usable8(T, hx, hy)


def _div(x, y):
    """x / y as IEEE does it (Python raises on a zero divisor; the walk only divides by values the usable test has bounded, the
    correction may meet a zero)"""
    try:
        return x / y
    except ZeroDivisionError:
        with np.errstate(all="ignore"):
            return float(np.float64(x) / np.float64(y))


def compose8(T, M):
    """T o M: M first, then T -- the 3 x 3 product, divided by its corner entry"""
    a = (T[0] * M[0] + T[1] * M[2]) + T[4] * M[6]
    b = (T[0] * M[1] + T[1] * M[3]) + T[4] * M[7]
    c = (T[2] * M[0] + T[3] * M[2]) + T[5] * M[6]
    d = (T[2] * M[1] + T[3] * M[3]) + T[5] * M[7]
    tx = (T[0] * M[4] + T[1] * M[5]) + T[4]
    ty = (T[2] * M[4] + T[3] * M[5]) + T[5]
    gx = (T[6] * M[0] + T[7] * M[2]) + M[6]
    gy = (T[6] * M[1] + T[7] * M[3]) + M[7]
    n = (T[6] * M[4] + T[7] * M[5]) + 1.0
    return tuple(_div(v, n) for v in (a, b, c, d, tx, ty, gx, gy))


def invert8(T):
    """the inverse of T: the adjugate divided by its corner entry D = a*d - b*c"""
    a, b, c, d, tx, ty, gx, gy = T
    D = a * d - b * c
    return tuple(_div(v, D) for v in (d - ty * gy, tx * gy - b, ty * gx - c, a - tx * gx, b * ty - tx * d, tx * c - a * ty,
                                      c * gy - d * gx, b * gx - a * gy))


def smoothed_map8(models, f, weights, hx, hy):
    """Q_f and the reach r_f of frame f under models [npairs][8]: smoothed_map's walk on eight numbers"""
    npairs = len(models)
    w0 = float(weights[0])
    acc = [w0, 0.0, 0.0, w0, 0.0, 0.0, 0.0, 0.0]
    sw = w0
    Mf = Mb = IDENTITY8
    r = 0
    with np.errstate(all="ignore"):
        for j in range(1, len(weights)):
            if f + j - 1 >= npairs or f - j < 0:
                break
            Tf, okf = pair_map8(models[f + j - 1], hx, hy)
            Tb, okb = pair_map8(models[f - j], hx, hy)
            if not (okf and okb):
                break
            Mf = compose8(Tf, Mf)
            Mb = compose8(invert8(Tb), Mb)
            wj = float(weights[j])
            acc = [acc[e] + (wj * Mf[e] + wj * Mb[e]) for e in range(8)]
            sw = sw + (wj + wj)
            r = j
    return tuple(v / sw for v in acc), r   # (sw >= w_0 > 0)


def correction8(Q, zoom, hx, hy):
    """the warp g [8] of a frame from its smoothed map: W = Q^-1 where Q is usable and Q^-1 is finite and usable, else the
    identity; zoomed about the centre"""
    W = IDENTITY8
    if usable8(Q, hx, hy):
        with np.errstate(all="ignore"):
            W = invert8(Q)
        if not usable8(W, hx, hy):
            W = IDENTITY8
    s = 1.0 / float(zoom)
    return (W[4], W[0] * s - 1.0, W[1] * s, W[5], W[2] * s, W[3] * s - 1.0, 0.0 - W[6] * s, 0.0 - W[7] * s)


def camera_path_projective_ref(models8, weights, zoom, w, h):
    """models8 [npairs][8] float64 (ofdis_projective_motion's parametrisation), weights [radius + 1] float64, the frame size ->
    warps [npairs + 1][8] float64, what ofdis_camera_path_projective writes"""
    weights = check_window(weights, zoom)
    hx, hy = half_sides(w, h)
    models8 = np.ascontiguousarray(models8, np.float64)
    assert models8.ndim == 2 and models8.shape[1] == 8 and models8.shape[0] >= 1, models8.shape
    warps = np.empty((models8.shape[0] + 1, 8), np.float64)
    for f in range(models8.shape[0] + 1):
        warps[f] = correction8(smoothed_map8(models8, f, weights, hx, hy)[0], zoom, hx, hy)
    return warps


def warp_positions8(g, w, h):
    """the sample positions of a warp g [8] (float64, converted to float32 first) and the sign test of the denominator:
    (px, py, front), float32 [h][w] twice and bool [h][w]"""
    X = (2 * np.arange(w, dtype=np.int64) - (w - 1))[None, :]
    Y = (2 * np.arange(h, dtype=np.int64) - (h - 1))[:, None]
    with np.errstate(all="ignore"):
        gf = np.asarray(g, np.float64).astype(_f32)
        xc, yc = X.astype(_f32) * _f32(0.5), Y.astype(_f32) * _f32(0.5)
        e = gf[6] * xc + gf[7] * yc
        D = _f32(1.0) - e
        r = _f32(1.0) / D
        mu = ((gf[0] + gf[1] * xc) + gf[2] * yc) + e * xc
        mv = ((gf[3] + gf[4] * xc) + gf[5] * yc) + e * yc
        px = np.arange(w, dtype=np.int64).astype(_f32)[None, :] + mu * r
        py = np.arange(h, dtype=np.int64).astype(_f32)[:, None] + mv * r
        front = D > _f32(0)
    assert px.dtype == _f32 and py.dtype == _f32 and px.shape == py.shape == front.shape == (h, w)
    return px, py, front


def warp_frames_projective_ref(frames, warps, border=BORDER_CONSTANT):
    """frames [n][h][w] (gray) or [n][h][w][3] uint8, warps [n][8] float64 -> (out, inside), the arrays
    ofdis_warp_frames_projective writes: warp_frames_ref with the positions of warp_positions8 and ins = front and inside(p)"""
    if border not in (BORDER_CONSTANT, BORDER_REPLICATE):
        raise ValueError("border must be BORDER_CONSTANT or BORDER_REPLICATE")
    frames = np.asarray(frames, np.uint8)
    gray = frames.ndim == 3
    I = frames[..., None] if gray else frames
    n, h, w, noc = I.shape
    assert noc in (1, 3) and max(w, h) <= GM_MAX_SIDE, frames.shape
    warps = np.asarray(warps, np.float64).reshape(n, 8)
    out, ins_out = np.empty_like(I), np.empty((n, h, w), np.uint8)
    for f in range(n):
        px, py, front = warp_positions8(warps[f], w, h)
        ins = front & _inside(px, py, w, h)
        pxc = np.fmin(np.fmax(px, _f32(0)), _f32(w - 1))
        pyc = np.fmin(np.fmax(py, _f32(0)), _f32(h - 1))
        c = _sample(I[f], pxc.ravel(), pyc.ravel()).reshape(h, w, noc)
        if border == BORDER_CONSTANT:
            c = np.where(ins[..., None], c, _f32(0))
        r = np.floor(c + _f32(0.5))
        assert r.dtype == _f32
        out[f] = np.clip(r.astype(np.int64), 0, 255).astype(np.uint8)
        ins_out[f] = ins
    return (out[..., 0] if gray else out), ins_out
