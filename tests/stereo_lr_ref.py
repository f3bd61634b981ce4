"""A numpy restatement of the stereo left-right step of include/ofdis.h (ofdis_lr_check, ofdis_disparity_fill and the
composition ofdis_batch_upsample_lr is defined as), float32, operation by operation in the documented order.  The GPU tests
compare the library with it bit for bit; tests/test_stereo_lr_abi.py runs it on the reference build's disparities."""
import numpy as np

CONSISTENT, INCONSISTENT, OUTSIDE = 0, 1, 2
FILL_NONE, FILL_INVALIDATE, FILL_BACKGROUND = 0, 1, 2
_f32 = np.float32


def mirror(img):
    """mir(I)[y][x] = I[y][W-1-x] for [..., h, w] or [..., h, w, c] frames given as (h, w[, c]) arrays."""
    return np.ascontiguousarray(img[:, ::-1])


def lr_check(disp, other, alpha=0.01, beta=0.5):
    """disp, other: [..., h, w] float32 -> uint8 codes."""
    d = np.ascontiguousarray(disp, _f32)
    R = np.ascontiguousarray(other, _f32)
    assert d.shape == R.shape
    W = d.shape[-1]
    alpha, beta = _f32(alpha), _f32(beta)
    with np.errstate(all="ignore"):
        x = np.arange(W, dtype=_f32)
        xb = x + d
        inside = (xb >= _f32(0)) & (xb <= _f32(W - 1))  # NaN: False
        xs = np.where(inside, xb, _f32(0))
        if W > 1:
            x0 = np.minimum(np.floor(xs).astype(np.int64), W - 2)
            ax = xs - x0.astype(_f32)
        else:
            x0 = np.zeros(d.shape, np.int64)
            ax = np.zeros(d.shape, _f32)
        x1 = np.minimum(x0 + 1, W - 1)
        bx = _f32(1) - ax
        r = np.take_along_axis(R, x0, -1) * bx + np.take_along_axis(R, x1, -1) * ax
        s = d + r
        lhs = s * s
        rhs = alpha * (d * d + r * r) + beta
        code = np.where(lhs <= rhs, CONSISTENT, INCONSISTENT)
    return np.where(inside, code, OUTSIDE).astype(np.uint8)


def _fill_row(d, cons):
    W = d.shape[0]
    out = d.copy()
    if not cons.any():
        return out
    idx = np.arange(W)
    left = np.maximum.accumulate(np.where(cons, idx, -1))                 # inclusive: == x on consistent pixels
    right = np.minimum.accumulate(np.where(cons, idx, W)[::-1])[::-1]
    with np.errstate(all="ignore"):
        for x in np.nonzero(~cons)[0]:
            l, r = left[x], right[x]
            if l >= 0 and r < W:
                out[x] = d[l] if np.abs(d[l]) <= np.abs(d[r]) else d[r]
            elif l >= 0:
                out[x] = d[l]
            else:
                out[x] = d[r]
    return out


def disparity_fill(disp, mask, mode):
    d = np.ascontiguousarray(disp, _f32)
    m = np.ascontiguousarray(mask, np.uint8)
    assert d.shape == m.shape
    if mode == FILL_NONE:
        return d.copy()
    if mode == FILL_INVALIDATE:
        return np.where(m != CONSISTENT, _f32(np.inf), d).astype(_f32)
    assert mode == FILL_BACKGROUND
    W = d.shape[-1]
    d2, m2 = d.reshape(-1, W), m.reshape(-1, W)
    out = np.stack([_fill_row(d2[i], m2[i] == CONSISTENT) for i in range(d2.shape[0])])
    return out.reshape(d.shape)


def right_view(dm):
    """DR[y][x] = -Dm[y][W-1-x] from the mirror pass's full-resolution disparity [..., h, w]."""
    return np.ascontiguousarray(-np.ascontiguousarray(dm, _f32)[..., ::-1])


def compose(u, dm, fill, alpha=0.01, beta=0.5):
    """The materialised composition: u = the forward disparity at full resolution, dm = the mirror pass's (both [..., h, w]).
    Returns (out_left, out_right, mask_left, mask_right); the masks are those of the unfilled disparities."""
    u = np.ascontiguousarray(u, _f32)
    dr = right_view(dm)
    ml, mr = lr_check(u, dr, alpha, beta), lr_check(dr, u, alpha, beta)
    return disparity_fill(u, ml, fill), disparity_fill(dr, mr, fill), ml, mr


def bits(a):
    return np.ascontiguousarray(a, _f32).view(np.uint32)
