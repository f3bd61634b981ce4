"""The level flow at full resolution for a free UpGeom, in numpy: what every level-form finish kernel recomputes on the fly
(of_dis_amd/csrc/ofdis_upsample.h) and what ofdis_batch_upsample_frames writes.  Written from the rule in the docstring of
tests/test_upsample_pin.py (OpenCV's INTER_LINEAR for float data), not from the device header:

    values times s = 2^sc_l; for a padded destination column X the source coordinate is fx = (X + 0.5) / s - 0.5; sx = floor(fx);
    fx -= sx; sx < 0 -> (sx, fx) = (0, 0); sx >= sw - 1 -> (sx, fx) = (sw - 1, 0); the row is interpolated horizontally,
    S[sx] * (1 - fx) + S[min(sx + 1, sw - 1)] * fx, then two such rows vertically by the same rule; then the crop of wo x ho at
    (left, top).

float32 throughout, every product and sum rounded on its own (s is a power of two, so the coordinates are exact).  A clamped
neighbour still enters with weight 0, so an infinite or NaN level value reaches every pixel that has it as one of its four
sources: inf * 0 = NaN.

Also here, shared by tests/test_up_ref.py (CPU) and tests/test_gpu_level_routes.py: the geometries the level routes are held to
(GEOMS), the product's crop rule (geom) and the three families of planted level flows (level_flows)."""
import functools

import numpy as np

from trajfilter_cases import coherent_case, random_case

_f32 = np.float32
NPAIRS = 4   # five frames


def geom(sw, sh, sc_l, wo, ho):
    """UpGeom (sw, sh, sc_l, left, top, wo, ho) as finish_begin (ofdis_products.hip) makes it for an original size wo x ho inside
    the padded size (sw << sc_l) x (sh << sc_l): the crop is centred, the odd pixel goes right and down"""
    W, H = sw << sc_l, sh << sc_l
    assert 1 <= wo <= W and 1 <= ho <= H, (sw, sh, sc_l, wo, ho)
    return (sw, sh, sc_l, (W - wo) // 2, (H - ho) // 2, wo, ho)


# (sw, sh, sc_l, wo, ho): the smallest geometries at which each class exists
GEOM_TABLE = [
    (9, 7, 0, 9, 7),       # x1, no crop
    (8, 5, 0, 5, 4),       # x1, asymmetric crop
    (5, 4, 1, 7, 5),       # wo % 4 == 3
    (5, 3, 2, 20, 12),     # no crop, 4-byte stores
    (5, 3, 2, 17, 9),      # odd crop
    (5, 3, 2, 14, 6),      # crop 3 > s/2: the clamped half group is gone on the left and top
    (4, 3, 3, 32, 24),     # full size
    (4, 3, 3, 27, 19),
    (4, 3, 3, 18, 13),     # crop 7 / 5: almost a whole level column
    (2, 2, 4, 29, 30),
    (3, 1, 4, 45, 13),     # sh == 1: every row clamped
    (1, 3, 4, 13, 44),     # sw == 1
    (1, 1, 3, 5, 1),       # ho == 1, top 3
    (2, 2, 1, 3, 3),       # wo < 4
    (1, 2, 2, 1, 6),       # wo == 1
    (12, 8, 3, 96, 61),    # more than one workgroup row of quads, several upsample_crop chunks per row
]
GEOMS = [geom(*t) for t in GEOM_TABLE]
GEOM_IDS = [f"{g[0]}x{g[1]}-x{1 << g[2]}-{g[5]}x{g[6]}" for g in GEOMS]
# a crop larger than s on both axes (x2, left = top = 3): whole level columns and rows are cropped away.  The padding is to
# 2^sc_f, not 2^sc_l, so contexts can make this; none of the geometries of GEOMS has it.  Held to the hand vectors and, on the
# GPU, to up_ref and the masks' definition
CROP_ABOVE_S = geom(6, 5, 1, 6, 4)
FAMILIES = ["wild", "coherent", "exact"]
# the integer translations of the exact family, one per pair: targets exactly on the last column / row from the pixel |t| before
# it, the camera models' validity bound |u| = 4096 met exactly, and no motion
EXACT_T = [(1, -1), (-3, 2), (4096, -4096), (0, 0)]
assert len(EXACT_T) == NPAIRS


def _axis(n_src, sc_l, first, count):
    """(index, clamped index + 1, fraction as float32) of padded destination coordinates first .. first + count - 1"""
    d = np.arange(first, first + count, dtype=np.int64)
    f = (d.astype(np.float64) + 0.5) / float(1 << sc_l) - 0.5   # exact in float32 as well: s is a power of two
    s0 = np.floor(f).astype(np.int64)
    frac = (f - s0).astype(_f32)
    assert np.array_equal(frac.astype(np.float64), f - s0)
    low, high = s0 < 0, s0 >= n_src - 1
    s0 = np.where(low, 0, np.where(high, n_src - 1, s0))
    frac = np.where(low | high, _f32(0), frac).astype(_f32)
    return s0, np.minimum(s0 + 1, n_src - 1), frac


def up_ref(level, g):
    """level [..., sh, sw, c] float32 (c = 1 or 2; leading axes are frames) -> [..., ho, wo, c] float32"""
    sw, sh, sc_l, left, top, wo, ho = g
    level = np.ascontiguousarray(level, _f32)
    assert level.ndim >= 3 and level.shape[-3:-1] == (sh, sw) and level.shape[-1] in (1, 2), (level.shape, g)
    sx, sx1, fx = _axis(sw, sc_l, left, wo)
    sy, sy1, fy = _axis(sh, sc_l, top, ho)
    fx, fy = fx[:, None], fy[:, None, None]
    one = _f32(1)
    with np.errstate(all="ignore"):
        v = level * _f32(1 << sc_l)
        rows = v[..., :, sx, :] * (one - fx) + v[..., :, sx1, :] * fx            # [..., sh, wo, c]
        out = rows[..., sy, :, :] * (one - fy) + rows[..., sy1, :, :] * fy         # [..., ho, wo, c]
    assert out.dtype == _f32
    return np.ascontiguousarray(out)


def up_ref1(level, g):
    """up_ref for one-channel planes (stereo disparities): level [..., sh, sw] -> [..., ho, wo]"""
    return np.ascontiguousarray(up_ref(np.asarray(level)[..., None], g)[..., 0])


@functools.lru_cache(maxsize=None)
def level_flows(g, family):
    """(fw, rev) [NPAIRS][sh][sw][2] float32, read-only: the planted level flows of a family at geometry g.  wild and coherent
    are the flows of tests/trajfilter_cases.py drawn at sw x sh and divided by 2^sc_l (exact), so that the full-resolution
    magnitudes stay what those families were built for; exact is the constant t / 2^sc_l per pair with rev = -fw, whose weights
    are all dyadic: the full-resolution flow is t at every pixel"""
    sw, sh, sc_l = g[:3]
    inv = _f32(1.0 / (1 << sc_l))
    if family == "exact":
        fw = np.empty((NPAIRS, sh, sw, 2), _f32)
        for k, t in enumerate(EXACT_T):
            fw[k] = np.asarray(t, _f32) * inv
        rev = -fw
    else:
        _, fw, rev = coherent_case(NPAIRS, sw, sh, 1) if family == "coherent" else random_case(NPAIRS, sw, sh, 1, family)
        with np.errstate(all="ignore"):
            fw, rev = fw * inv, rev * inv
    for a in (fw, rev):
        a.setflags(write=False)
    return fw, rev


def exact_masks(g):
    """the closed form of both masks of the exact family [NPAIRS][ho][wo] uint8: 2 (outside) on the band of |t| columns / rows
    whose target leaves the image, 0 (consistent) elsewhere -- fw + rev = 0 at every target"""
    wo, ho = g[5], g[6]
    ys, xs = np.mgrid[0:ho, 0:wo]
    out = []
    for sign in (1, -1):
        m = np.empty((NPAIRS, ho, wo), np.uint8)
        for k, (tx, ty) in enumerate(EXACT_T):
            qx, qy = xs + sign * tx, ys + sign * ty
            m[k] = np.where((qx >= 0) & (qx <= wo - 1) & (qy >= 0) & (qy <= ho - 1), 0, 2)
        out.append(m)
    return out
