"""Numpy model of the global motion models and the motion-compensated flow of include/ofdis.h (ofdis_global_motion,
ofdis_motion_compensate and their ofdis_batch_* twins): the header's definition in its order -- the twelve sums as exact int64,
the solve in float64 and the residual in float32, one rounding per operation.  Needs numpy only (no GPU, no library): the tests
compare the kernels against `global_motion_ref` and `motion_compensate_ref` bit for bit.

    from of_dis_amd import gmotion
    models, stats = gmotion.global_motion_ref(flow, mask, model=gmotion.GM_AFFINE, rounds=3, thresh=1.0)
    residual, label = gmotion.motion_compensate_ref(flow, models, mask, thresh=1.0)
    foreground = label == gmotion.GM_OUTLIER

The 8-parameter projective models (ofdis_projective_motion, ofdis_projective_compensate) share the round loop, the
compensation, the term table of the sums, the residual and the model field with the 6-parameter ones, switched on the model's
width; their sums and solve (`sums23`, `solve8`) are stated at the end of the file, with `projective_motion_ref`,
`projective_compensate_ref` and `homography`.
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


def _terms(flow, sel, perm, nsums):
    """the per-pixel terms of the first `nsums` sums (12 or PM_NSUMS) over the pixels `sel`, in the record order: int64 arrays"""
    h, w = sel.shape
    X, Y = coords(w, h)
    X, Y = X[sel], Y[sel]
    q = np.rint(flow[sel] * _f32(256.0)).astype(np.int64)   # (the product is exact; np.rint rounds to nearest even, like rintf)
    qu, qv = q[:, 0], q[:, 1]
    if perm is not None:
        X, Y, qu, qv = X[perm], Y[perm], qu[perm], qv[perm]
    XX, XY, YY = X * X, X * Y, Y * Y
    terms = [np.ones_like(X), X, Y, XX, XY, YY, qu, X * qu, Y * qu, qv, X * qv, Y * qv]
    if nsums > 12:
        terms += [XX * X, XX * Y, X * YY, YY * Y, XX * XX, XX * XY, XX * YY, XY * YY, YY * YY, XX * qu + XY * qv, XY * qu + YY * qv]
    return terms


def sums(flow, sel, perm=None):
    """The twelve sums over the pixels `sel` (bool [h][w], all valid) as Python ints, in the record order n, SX, SY, SXX, SXY,
    SYY, Squ, SXqu, SYqu, Sqv, SXqv, SYqv.  perm: a permutation of the selected pixels applied before the summation (integer
    addition is associative: the tests use it to show that the order cannot matter)."""
    return [int(t.sum(dtype=np.int64)) for t in _terms(flow, sel, perm, 12)]


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
    """flow [h][w][2] float32 minus the model a [6] or [8] (float64, converted to float32 first): [h][w][2] float32"""
    h, w = flow.shape[:2]
    X, Y = coords(w, h)
    with np.errstate(over="ignore", invalid="ignore"):
        af = np.asarray(a, np.float64).astype(_f32)
        xc, yc = X.astype(_f32) * _f32(0.5), Y.astype(_f32) * _f32(0.5)
        mu = (af[0] + af[1] * xc) + af[2] * yc
        mv = (af[3] + af[4] * xc) + af[5] * yc
        if af.size == 8:
            p = af[6] * xc + af[7] * yc
            mu, mv = mu + p * xc, mv + p * yc
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


def _fit_ref(nparam, flow, mask, model, rounds, thresh, shuffle):
    """the rounds of a fit with models of nparam doubles: (models [npairs][nparam] float64, stats [npairs][3] int64)"""
    flow, mask = _pairs(flow, mask)
    models = np.zeros((flow.shape[0], nparam), np.float64)
    stats = np.zeros((flow.shape[0], 3), np.int64)
    for k in range(flow.shape[0]):
        ok = valid(flow[k], None if mask is None else mask[k])
        sel = ok
        for r in range(rounds):
            if r > 0:
                sel = near(residual(flow[k], models[k]), ok, thresh)
            perm = None if shuffle is None else shuffle.permutation(int(sel.sum()))
            s = sums(flow[k], sel, perm) if nparam == 6 else sums23(flow[k], sel, perm)
            if r > 0 and s[0] == 0:
                break   # the model, set size and status (or count) of round r-1 stay
            models[k], status = solve(s, model) if nparam == 6 else solve8(s)
            if r == 0:
                stats[k, 0] = s[0]
            stats[k, 1:] = s[0], status
    return models, stats


def _compensate_ref(nparam, flow, models, mask, thresh):
    _check(1, thresh)
    flow, mask = _pairs(flow, mask)
    models = np.asarray(models, np.float64).reshape(flow.shape[0], nparam)
    res = np.empty_like(flow)
    label = np.empty(flow.shape[:3], np.uint8)
    for k in range(flow.shape[0]):
        ok = valid(flow[k], None if mask is None else mask[k])
        res[k] = residual(flow[k], models[k])
        label[k] = np.where(near(res[k], ok, thresh), GM_INLIER, np.where(ok, GM_OUTLIER, GM_INVALID))
    return res, label


def global_motion_ref(flow, mask=None, model=GM_AFFINE, rounds=3, thresh=1.0, shuffle=None):
    """flow [npairs][h][w][2] float32, mask [npairs][h][w] uint8 or None -> (models [npairs][6] float64, stats [npairs][3]
    int64: |S_0|, the size of the last set used, the status), what ofdis_global_motion writes.  shuffle: a
    numpy.random.Generator that permutes the pixels of every sum (the result must not change)."""
    _check(rounds, thresh)
    if model not in (GM_TRANSLATION_ONLY, GM_AFFINE):
        raise ValueError("model must be GM_TRANSLATION_ONLY or GM_AFFINE")
    return _fit_ref(6, flow, mask, model, rounds, thresh, shuffle)


def motion_compensate_ref(flow, models, mask=None, thresh=1.0):
    """flow [npairs][h][w][2] float32, models [npairs][6] float64 -> (residual [npairs][h][w][2] float32, label [npairs][h][w]
    uint8), what ofdis_motion_compensate writes."""
    return _compensate_ref(6, flow, models, mask, thresh)


def model_flow(a, w, h):
    """the model's flow field [h][w][2] in float64: u = a0 + a1*(x - cx) + a2*(y - cy), v likewise, and for a [8] the quadratic
    terms stated below (for users and tests; the kernels use `residual`)"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    xs -= (w - 1) / 2.0
    ys -= (h - 1) / 2.0
    if len(a) == 6:
        return np.stack([a[0] + a[1] * xs + a[2] * ys, a[3] + a[4] * xs + a[5] * ys], axis=-1)
    p = a[6] * xs + a[7] * ys
    return np.stack([a[0] + a[1] * xs + a[2] * ys + p * xs, a[3] + a[4] * xs + a[5] * ys + p * ys], axis=-1)


# ------------------------------------------------------------------ 8-parameter projective models (ofdis_projective_motion)
# include/ofdis.h, "Projective camera models": the quadratic (first-order projective) flow model
#     p = a6*xc + a7*yc;  u = a0 + a1*xc + a2*yc + p*xc;  v = a3 + a4*xc + a5*yc + p*yc
# fitted from 23 exact integer sums.  In integer units b (u_q = b0 + b1 X + b2 Y + b6 X^2 + b7 XY, v_q = b3 + b4 X + b5 Y +
# b6 XY + b7 Y^2) the normal matrix N is
#     rows / columns 0..2 and 3..5: [[n, SX, SY], [SX, SXX, SXY], [SY, SXY, SYY]], zero between the two blocks
#     column 6: (SXX, XXX, XXY, SXY, XXY, XYY), N66 = XXXX + XXYY     column 7: (SXY, XXY, XYY, SYY, XYY, YYY), N77 = XXYY + YYYY
#     N67 = XXXY + XYYY
# and the right-hand side t = (Squ, SXqu, SYqu, Sqv, SXqv, SYqv, R6, R7).  Every sum is converted to float64 correctly rounded
# (float(int)), the three sums of N66, N67, N77 are float64 additions.  Then, every operation rounded on its own:
#     for k = 0..7:  for i = k..7:  C_ik = N_ik;  for j = 0..k-1 ascending: C_ik = C_ik - C_ij * L_kj
#                    d_k = C_kk;  the pivot passes when d_k > N_kk * 2^-40;  for i = k+1..7: L_ik = C_ik / d_k
#     z_i = t_i;  for j = 0..i-1 ascending: z_i = z_i - L_ij * z_j         (i = 0..7)
#     y_i = z_i / d_i
#     b_i = y_i;  for j = i+1..7 ascending: b_i = b_i - L_ji * b_j         (i = 7..0)
#     a0 = b0/256, a1 = b1/128, a2 = b2/128, a3 = b3/256, a4 = b4/128, a5 = b5/128, a6 = b6/64, a7 = b7/64
# The projective branch is taken when n >= 4 and all eight pivots pass; otherwise `solve(s[:12], GM_AFFINE)` decides, a6 = a7 = 0.
PM_NSUMS = 23           # the sums of a record (padded to PM_RECORD int64 in the work buffer)
PM_RECORD = 24
PM_BLOCK_PIXELS = 1024  # a workgroup's share of a pair: 256 quads of 4 pixels
PM_PIVOT = 2.0 ** -40
_PM_COUNT = {GM_OK_AFFINE: 6, GM_TRANSLATION: 2, GM_EMPTY: 0}


def sums23(flow, sel, perm=None, chunk=PM_BLOCK_PIXELS):
    """The 23 sums over the pixels `sel` as Python ints, in the record order: the twelve of `sums`, then XXX, XXY, XYY, YYY,
    XXXX, XXXY, XXYY, XYYY, YYYY, R6 = sum(X*X*qu + X*Y*qv), R7 = sum(X*Y*qu + Y*Y*qv).  Chunks of at most `chunk` pixels
    (a workgroup's 1024) are summed in int64, as the accumulate kernel does, and the chunks are added as Python ints, as the
    solve kernel's 128-bit sums are.  perm: as in `sums`."""
    assert chunk <= PM_BLOCK_PIXELS
    return [sum(int(t[c0:c0 + chunk].sum(dtype=np.int64)) for c0 in range(0, len(t), chunk))
            for t in _terms(flow, sel, perm, PM_NSUMS)]


def normal8(s):
    """the normal matrix (8 rows of 8 floats) and right-hand side of the 23 sums, as stated above"""
    f = [float(v) for v in s]
    n, Sx, Sy, Sxx, Sxy, Syy = f[:6]
    xxx, xxy, xyy, yyy, x4, x3y, x2y2, xy3, y4 = f[12:21]
    M = [[n, Sx, Sy], [Sx, Sxx, Sxy], [Sy, Sxy, Syy]]
    N = [[0.0] * 8 for _ in range(8)]
    for i in range(3):
        for j in range(3):
            N[i][j] = N[3 + i][3 + j] = M[i][j]
    col6 = [Sxx, xxx, xxy, Sxy, xxy, xyy]
    col7 = [Sxy, xxy, xyy, Syy, xyy, yyy]
    for i in range(6):
        N[i][6] = N[6][i] = col6[i]
        N[i][7] = N[7][i] = col7[i]
    N[6][6] = x4 + x2y2
    N[6][7] = N[7][6] = x3y + xy3
    N[7][7] = x2y2 + y4
    return N, f[6:12] + f[21:23]


def solve8(s):
    """The header's solve on the 23 sums: (a [8] float64, count), count = 8, 6, 2 or 0 parameters solved.  pivot_ratios(s)
    gives the d_k / N_kk the rank test looks at."""
    b = _ldl8(s)[0] if s[0] >= 4 else None
    if b is not None:
        a = [b[0] / 256.0, b[1] / 128.0, b[2] / 128.0, b[3] / 256.0, b[4] / 128.0, b[5] / 128.0, b[6] / 64.0, b[7] / 64.0]
        return np.array(a, np.float64), 8
    a6, status = solve(s[:12], GM_AFFINE)
    return np.concatenate([a6, np.zeros(2)]), _PM_COUNT[status]


def _ldl8(s):
    """(b [8] or None where a pivot fails, the pivots d_k computed so far, the diagonal N_kk)"""
    N, t = normal8(s)
    C = [[0.0] * 8 for _ in range(8)]
    L = [[0.0] * 8 for _ in range(8)]
    d = []
    for k in range(8):
        for i in range(k, 8):
            acc = N[i][k]
            for j in range(k):
                acc = acc - C[i][j] * L[k][j]
            C[i][k] = acc
        d.append(C[k][k])
        if not d[k] > N[k][k] * PM_PIVOT:
            return None, d, [N[i][i] for i in range(8)]
        for i in range(k + 1, 8):
            L[i][k] = C[i][k] / d[k]
    z = list(t)
    for i in range(8):
        for j in range(i):
            z[i] = z[i] - L[i][j] * z[j]
    b = [z[i] / d[i] for i in range(8)]
    for i in range(7, -1, -1):
        for j in range(i + 1, 8):
            b[i] = b[i] - L[j][i] * b[j]
    return b, d, [N[i][i] for i in range(8)]


def pivot_ratios(s):
    """d_k / N_kk of the pivots the factorisation reached (the last one is the failing one where the rank test fails)"""
    _, d, diag = _ldl8(s)
    return [dk / nk if nk else 0.0 for dk, nk in zip(d, diag)]


residual8 = residual      # (the width of the model decides)
model_flow8 = model_flow


def projective_motion_ref(flow, mask=None, rounds=3, thresh=1.0, shuffle=None):
    """flow [npairs][h][w][2] float32, mask [npairs][h][w] uint8 or None -> (models [npairs][8] float64, stats [npairs][3]
    int64: |S_0|, the size of the last set used, the number of parameters solved: 8, 6, 2 or 0), what ofdis_projective_motion
    writes.  shuffle: as in global_motion_ref."""
    _check(rounds, thresh)
    return _fit_ref(8, flow, mask, None, rounds, thresh, shuffle)


def projective_compensate_ref(flow, models, mask=None, thresh=1.0):
    """flow [npairs][h][w][2] float32, models [npairs][8] float64 -> (residual [npairs][h][w][2] float32, label [npairs][h][w]
    uint8), what ofdis_projective_compensate writes."""
    return _compensate_ref(8, flow, models, mask, thresh)


def homography(a):
    """the homography the model a [8] is the first-order flow of, in centred coordinates: [[1+a1, a2, a0], [a4, 1+a5, a3],
    [-a6, -a7, 1]] (float64 [3][3]); a 6-parameter model gives the affine matrix"""
    a = np.concatenate([np.asarray(a, np.float64).ravel(), np.zeros(2)])[:8]
    return np.array([[1.0 + a[1], a[2], a[0]], [a[4], 1.0 + a[5], a[3]], [-a[6], -a[7], 1.0]], np.float64)
