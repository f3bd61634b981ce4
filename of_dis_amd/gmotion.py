"""Numpy model of the global motion models and the motion-compensated flow of include/ofdis.h (ofdis_global_motion,
ofdis_motion_compensate and their ofdis_batch_* twins): the header's definition in its order -- the twelve sums as exact int64,
the solve in float64 and the residual in float32, one rounding per operation.  Needs numpy only (no GPU, no library): the tests
compare the kernels against `global_motion_ref` and `motion_compensate_ref` bit for bit.

    from of_dis_amd import gmotion
    models, stats = gmotion.global_motion_ref(flow, mask, model=gmotion.GM_AFFINE, rounds=3, thresh=1.0)
    residual, label = gmotion.motion_compensate_ref(flow, models, mask, thresh=1.0)
    foreground = label == gmotion.GM_OUTLIER
"""
import numpy as np

GM_MAX_SIDE, GM_MAX_FLOW, GM_MAX_ROUNDS = 8192, 4096.0, 8   # include/ofdis.h: OFDIS_GM_MAX_*
GM_TRANSLATION_ONLY, GM_AFFINE = 0, 1                        # model
GM_OK_AFFINE, GM_TRANSLATION, GM_EMPTY = 0, 1, 2             # status
GM_INLIER, GM_OUTLIER, GM_INVALID = 0, 1, 2                  # label
FB_CONSISTENT = 0  # include/ofdis.h: OFDIS_FB_CONSISTENT (capi.FB_CONSISTENT)

_f32 = np.float32


def coords(w, h):
    """the centred, doubled integer coordinates X = 2x - (w-1), Y = 2y - (h-1) of every pixel: two int64 arrays [h][w]"""
    X = 2 * np.arange(w, dtype=np.int64) - (w - 1)
    Y = 2 * np.arange(h, dtype=np.int64) - (h - 1)
    return np.broadcast_to(X[None, :], (h, w)), np.broadcast_to(Y[:, None], (h, w))


def valid(flow, mask=None):
    """flow [h][w][2] float32, mask [h][w] uint8 or None: bool [h][w]"""
    with np.errstate(invalid="ignore"):
        ok = (np.abs(flow[..., 0]) <= _f32(GM_MAX_FLOW)) & (np.abs(flow[..., 1]) <= _f32(GM_MAX_FLOW))
    if mask is not None:
        ok &= mask == FB_CONSISTENT
    return ok


def sums(flow, sel, perm=None):
    """The twelve sums over the pixels `sel` (bool [h][w], all valid) as Python ints, in the record order n, SX, SY, SXX, SXY,
    SYY, Squ, SXqu, SYqu, Sqv, SXqv, SYqv.  perm: a permutation of the selected pixels applied before the summation (integer
    addition is associative: the tests use it to show that the order cannot matter)."""
    h, w = sel.shape
    X, Y = coords(w, h)
    X, Y = X[sel], Y[sel]
    uv = flow[sel]
    q = np.rint(uv * _f32(256.0)).astype(np.int64)   # (the product is exact; np.rint rounds to nearest even, like rintf)
    qu, qv = q[:, 0], q[:, 1]
    if perm is not None:
        X, Y, qu, qv = X[perm], Y[perm], qu[perm], qv[perm]
    terms = [np.ones_like(X), X, Y, X * X, X * Y, Y * Y, qu, X * qu, Y * qu, qv, X * qv, Y * qv]
    return [int(t.sum(dtype=np.int64)) for t in terms]


def solve(s, model):
    """The header's solve on the twelve sums: (a [6] float64, status).  Python floats are IEEE doubles and every operation
    below is rounded on its own; int -> float is the correctly rounded conversion."""
    a = [0.0] * 6
    if s[0] == 0:
        return np.array(a, np.float64), GM_EMPTY
    n, Sx, Sy, Sxx, Sxy, Syy = (float(v) for v in s[:6])
    S = [[float(v) for v in s[6:9]], [float(v) for v in s[9:12]]]
    if model == GM_AFFINE and s[0] >= 3:
        c00 = Sxx * Syy - Sxy * Sxy
        c01 = Sxy * Sy - Sx * Syy
        c02 = Sx * Sxy - Sxx * Sy
        c11 = n * Syy - Sy * Sy
        c12 = Sx * Sy - n * Sxy
        c22 = n * Sxx - Sx * Sx
        det = (n * c00 + Sx * c01) + Sy * c02
        if det > 0.0:
            for c, (Su, Sxu, Syu) in enumerate(S):
                b0 = ((c00 * Su + c01 * Sxu) + c02 * Syu) / det
                b1 = ((c01 * Su + c11 * Sxu) + c12 * Syu) / det
                b2 = ((c02 * Su + c12 * Sxu) + c22 * Syu) / det
                a[3 * c], a[3 * c + 1], a[3 * c + 2] = b0 / 256.0, b1 / 128.0, b2 / 128.0
            return np.array(a, np.float64), GM_OK_AFFINE
    a[0] = (S[0][0] / n) / 256.0
    a[3] = (S[1][0] / n) / 256.0
    return np.array(a, np.float64), GM_TRANSLATION


def residual(flow, a):
    """flow [h][w][2] float32 minus the model a [6] (float64, converted to float32 first): [h][w][2] float32"""
    h, w = flow.shape[:2]
    X, Y = coords(w, h)
    with np.errstate(over="ignore", invalid="ignore"):
        af = np.asarray(a, np.float64).astype(_f32)
        xc, yc = X.astype(_f32) * _f32(0.5), Y.astype(_f32) * _f32(0.5)
        mu = (af[0] + af[1] * xc) + af[2] * yc
        mv = (af[3] + af[4] * xc) + af[5] * yc
        return np.stack([flow[..., 0] - mu, flow[..., 1] - mv], axis=-1)


def near(res, ok, thresh):
    """valid and ru*ru + rv*rv <= thresh*thresh, all float32 (NaN: False)"""
    t2 = _f32(thresh) * _f32(thresh)
    with np.errstate(over="ignore", invalid="ignore"):
        r2 = res[..., 0] * res[..., 0] + res[..., 1] * res[..., 1]
        return ok & (r2 <= t2)


def _check(rounds, thresh):
    if not 1 <= rounds <= GM_MAX_ROUNDS:
        raise ValueError("rounds outside 1..GM_MAX_ROUNDS")
    if not (np.isfinite(thresh) and thresh > 0):
        raise ValueError("thresh must be finite and > 0")


def _pairs(flow, mask):
    flow = np.ascontiguousarray(flow, _f32)
    assert flow.ndim == 4 and flow.shape[-1] == 2, flow.shape
    assert max(flow.shape[1:3]) <= GM_MAX_SIDE, flow.shape
    if mask is not None:
        mask = np.ascontiguousarray(mask, np.uint8)
        assert mask.shape == flow.shape[:3], (mask.shape, flow.shape)
    return flow, mask


def global_motion_ref(flow, mask=None, model=GM_AFFINE, rounds=3, thresh=1.0, shuffle=None):
    """flow [npairs][h][w][2] float32, mask [npairs][h][w] uint8 or None -> (models [npairs][6] float64, stats [npairs][3]
    int64: |S_0|, the size of the last set used, the status), what ofdis_global_motion writes.  shuffle: a
    numpy.random.Generator that permutes the pixels of every sum (the result must not change)."""
    _check(rounds, thresh)
    if model not in (GM_TRANSLATION_ONLY, GM_AFFINE):
        raise ValueError("model must be GM_TRANSLATION_ONLY or GM_AFFINE")
    flow, mask = _pairs(flow, mask)
    models = np.zeros((flow.shape[0], 6), np.float64)
    stats = np.zeros((flow.shape[0], 3), np.int64)
    for k in range(flow.shape[0]):
        ok = valid(flow[k], None if mask is None else mask[k])
        sel = ok
        for r in range(rounds):
            if r > 0:
                sel = near(residual(flow[k], models[k]), ok, thresh)
            s = sums(flow[k], sel, None if shuffle is None else shuffle.permutation(int(sel.sum())))
            if r > 0 and s[0] == 0:
                break   # the model, set size and status of round r-1 stay
            models[k], status = solve(s, model)
            if r == 0:
                stats[k, 0] = s[0]
            stats[k, 1:] = s[0], status
    return models, stats


def motion_compensate_ref(flow, models, mask=None, thresh=1.0):
    """flow [npairs][h][w][2] float32, models [npairs][6] float64 -> (residual [npairs][h][w][2] float32, label [npairs][h][w]
    uint8), what ofdis_motion_compensate writes."""
    _check(1, thresh)
    flow, mask = _pairs(flow, mask)
    models = np.asarray(models, np.float64).reshape(flow.shape[0], 6)
    res = np.empty_like(flow)
    label = np.empty(flow.shape[:3], np.uint8)
    for k in range(flow.shape[0]):
        ok = valid(flow[k], None if mask is None else mask[k])
        res[k] = residual(flow[k], models[k])
        label[k] = np.where(near(res[k], ok, thresh), GM_INLIER, np.where(ok, GM_OUTLIER, GM_INVALID))
    return res, label


def model_flow(a, w, h):
    """the model's flow field [h][w][2] in float64: u = a0 + a1*(x - cx) + a2*(y - cy), v likewise (for users and tests; the
    kernels use `residual`)"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    xs -= (w - 1) / 2.0
    ys -= (h - 1) / 2.0
    return np.stack([a[0] + a[1] * xs + a[2] * ys, a[3] + a[4] * xs + a[5] * ys], axis=-1)
