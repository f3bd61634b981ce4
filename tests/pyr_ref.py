"""An exact reference of the image pyramid (of_dis_amd/csrc/ofdis_pyr.hip), written from its definition in numpy alone -- not from
the kernels and not from oracle/ofdis_oracle.c, so that the three can be held against each other bit for bit.

The definition.  A frame of wo x ho 8-bit pixels is replicate-padded to the working size W x H, floor((W - wo) / 2) columns on
the left and floor((H - ho) / 2) rows on top.  The image of level l is the mean of every 2^l x 2^l block of that padded frame:
an integer block sum (int64 here) divided by 4^l.  Its gradients are the 3 x 3 Sobel operator scaled by 1/8 with the
reflect-101 border (one reflection; an axis of one pixel repeats its pixel).  The planes a level hands on are the image padded
by `pad` with its edge pixels and the gradients padded by `pad` with zeros.

Exactness.  Everything above is computed in int64 and float64, and every value is ASSERTED to be exactly representable in
float32 before it is cast (f32_exact): that is the claim of the header of ofdis_pyr.hip (8 + 2 l significant bits for a level
image, two more for a gradient, exact up to l = 7), checked on every input a test uses.  With it no summation order matters
and every comparison against this module is bit equality.

The per-stage functions (base, down, planes) take what the launchers take, so a test can check one stage on its own.  On
float input that is not 8-bit-derived, down() and planes() compute in float32 in the order the kernels state:
    down:  ((a + b) + (c + d)) * 0.25              a b / c d the 2 x 2 block
    dx:    ((r0 + 2 r1) + r2) * 0.125              r_j = right - left neighbour in window row j
    dy:    ((c0 + 2 c1) + c2) * 0.125              c_i = lower - upper neighbour in window column i
so bits still compare; on 8-bit-derived input they are asserted equal to the float64 definition."""
import numpy as np

_f32, _f64 = np.float32, np.float64


def f32_exact(a, what):
    """the float64 array `a` as float32, after asserting that no value changes by the cast (signed zeros included)"""
    a = np.asarray(a, _f64)
    b = a.astype(_f32)
    assert np.array_equal(b.astype(_f64), a) and np.array_equal(np.signbit(b), np.signbit(a)), \
        f"{what}: {int((b.astype(_f64) != a).sum())} values are not representable in float32 -- outside the exactness domain"
    return b


def _hwc(img):
    img = np.asarray(img)
    return img[:, :, None] if img.ndim == 2 else img


def pad_frame(img_u8, W, H):
    """[ho][wo]([noc]) -> [H][W][noc] uint8, replicate-padded: floor of the missing columns left, floor of the rows on top"""
    img = _hwc(img_u8)
    ho, wo = img.shape[:2]
    assert img.dtype == np.uint8 and 1 <= wo <= W and 1 <= ho <= H
    ys = np.clip(np.arange(H) - (H - ho) // 2, 0, ho - 1)
    xs = np.clip(np.arange(W) - (W - wo) // 2, 0, wo - 1)
    return img[ys][:, xs]


def level_image(padded_u8, l):
    """the unpadded image of level l as float64: int64 sums of the 2^l x 2^l blocks of [H][W][noc], divided by 4^l"""
    H, W, noc = padded_u8.shape
    bs = 1 << l
    h, w = H >> l, W >> l
    sums = padded_u8[:h * bs, :w * bs].astype(np.int64).reshape(h, bs, w, bs, noc).sum(axis=(1, 3))
    return sums.astype(_f64) / _f64(4 ** l)


def _reflect101(n):
    """(minus, plus): the indices of the neighbours -1 and +1 along an axis of n pixels under reflect-101"""
    i = np.arange(n)
    if n == 1:
        return i, i
    return np.where(i > 0, i - 1, 1), np.where(i < n - 1, i + 1, n - 2)


def sobel(v):
    """(dx, dy) of [h][w][noc] in float64, from the definition: the separable form (a central difference along one axis, the
    1 2 1 smoothing along the other) divided by 8"""
    v = np.asarray(v, _f64)
    ym, yp = _reflect101(v.shape[0])
    xm, xp = _reflect101(v.shape[1])
    d = v[:, xp] - v[:, xm]
    s = v[:, xm] + 2.0 * v + v[:, xp]
    return (d[ym] + 2.0 * d + d[yp]) / 8.0, (s[yp] - s[ym]) / 8.0


def sobel_f32(v):
    """(dx, dy) of float32 [h][w][noc] in float32, in the operation order of the kernels (module docstring)"""
    v = np.asarray(v, _f32)
    ym, yp = _reflect101(v.shape[0])
    xm, xp = _reflect101(v.shape[1])
    two, eighth = _f32(2.0), _f32(0.125)
    r = v[:, xp] - v[:, xm]            # right - left, per row
    c = v[yp] - v[ym]                  # lower - upper, per column
    dx = ((r[ym] + two * r) + r[yp]) * eighth
    dy = ((c[:, xm] + two * c) + c[:, xp]) * eighth
    assert dx.dtype == _f32 and dy.dtype == _f32
    return dx, dy


def _is_exact_domain(v):
    """8-bit-derived data: multiples of 4^-7 below 256, on which every sum above is exact in float32"""
    s = np.asarray(v, _f64) * 4.0 ** 7
    return bool(np.isfinite(s).all() and (s == np.round(s)).all() and (np.abs(np.asarray(v, _f64)) <= 255).all())


def pad_planes(image, dx, dy, pad):
    """[h][w][noc] -> [h + 2 pad][w + 2 pad][noc]: the image with its edge replicated, the gradients with zeros"""
    p = ((pad, pad), (pad, pad), (0, 0))
    return np.pad(image, p, mode="edge"), np.pad(dx, p, mode="constant"), np.pad(dy, p, mode="constant")


def pyramid(img_u8, W, H, levels, pad):
    """{l: (image, dx, dy, unpadded_image)} as float32 for l in `levels`: the padded planes [H/2^l + 2 pad][W/2^l + 2 pad][noc]
    and the unpadded level image [H/2^l][W/2^l][noc] of one frame [ho][wo]([noc]) uint8 at the working size W x H"""
    padded = pad_frame(img_u8, W, H)
    out = {}
    for l in levels:
        assert W % (1 << l) == 0 and H % (1 << l) == 0, (W, H, l)
        v = level_image(padded, l)
        gx, gy = sobel(v)
        what = f"level {l} of {img_u8.shape} in {W}x{H}"
        v32, gx32, gy32 = f32_exact(v, what + ", image"), f32_exact(gx, what + ", dx"), f32_exact(gy, what + ", dy")
        out[l] = pad_planes(v32, gx32, gy32, pad) + (v32,)
    return out


# ------------------------------------------------------------------ the stages, with the launchers' arguments
def frames_of(buf, nframes, wo, ho, noc, pitch, stride, offset=0):
    """[nframes][ho][wo][noc] uint8 out of the bytes `buf`: row y of frame f starts at offset + f * stride + y * pitch and has
    wo * noc bytes -- what lies between rows and between frames is not looked at"""
    buf = np.asarray(buf, np.uint8).ravel()
    out = np.empty((nframes, ho, wo * noc), np.uint8)
    for f in range(nframes):
        for y in range(ho):
            o = offset + f * stride + y * pitch
            assert o + wo * noc <= buf.size
            out[f, y] = buf[o:o + wo * noc]
    return out.reshape(nframes, ho, wo, noc)


def base(buf, nframes, wo, ho, W, H, noc, l, pitch, stride, offset=0):
    """launch_pyr_base: the unpadded level-l images [nframes][H >> l][W >> l][noc] float32 of the frames in `buf`"""
    frames = frames_of(buf, nframes, wo, ho, noc, pitch, stride, offset)
    return np.stack([f32_exact(level_image(pad_frame(f, W, H), l), f"base level {l}, frame {k}") for k, f in enumerate(frames)])


def down(src):
    """launch_pyr_down: [n][h][w][noc] float32 -> [n][h / 2][w / 2][noc], the mean of every 2 x 2 block (a last odd row or
    column is ignored)"""
    src = np.asarray(src, _f32)
    n, h, w, noc = src.shape
    h2, w2 = h // 2, w // 2
    s = src[:, :2 * h2, :2 * w2]
    a, b, c, d = s[:, 0::2, 0::2], s[:, 0::2, 1::2], s[:, 1::2, 0::2], s[:, 1::2, 1::2]
    out = ((a + b) + (c + d)) * _f32(0.25)
    assert out.dtype == _f32 and out.shape == (n, h2, w2, noc)
    if _is_exact_domain(src):   # the definition: an exact mean
        mean = s.astype(_f64).reshape(n, h2, 2, w2, 2, noc).sum(axis=(2, 4)) / 4.0
        assert np.array_equal(out.astype(_f64), mean), "down: the float32 order differs from the exact mean on 8-bit-derived data"
    return out


def planes(src, pad, gradients=True):
    """launch_pyr_planes: (image, dx, dy) [n][h + 2 pad][w + 2 pad][noc] float32 of the unpadded level images [n][h][w][noc];
    dx = dy = None without gradients"""
    src = np.asarray(src, _f32)
    assert src.ndim == 4
    exact = _is_exact_domain(src)
    out = [[], [], []]
    for k, v in enumerate(src):
        gx, gy = sobel_f32(v)
        if exact:   # the definition in float64, representable, and the same bits
            ex, ey = sobel(v)
            assert np.array_equal(f32_exact(ex, f"planes dx, frame {k}"), gx) and np.array_equal(f32_exact(ey, f"planes dy, frame {k}"), gy)
        for o, a in zip(out, pad_planes(v, gx, gy, pad)):
            o.append(a)
    img, dx, dy = (np.stack(o) for o in out)
    return (img, dx, dy) if gradients else (img, None, None)
