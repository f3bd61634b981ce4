"""What the tests of the projective stabiliser share (tests/test_stabilize_projective_ref.py on the CPU,
tests/test_gpu_stabilize_projective.py on the device): the generated 8-parameter models and warps, and the rotating-camera
clip of the end-to-end test with its metric.  A plain module like seq_products.py: no fixtures, needs numpy and scipy only."""
import functools
import math

import numpy as np

from of_dis_amd import gmotion, stabilize

_SCALE8 = np.array([3.0, 0.02, 0.02, 3.0, 0.02, 0.02, 1e-4, 1e-4])


# ------------------------------------------------------------------ models of the camera path
@functools.lru_cache(maxsize=None)
def models8(npairs, kind):
    """the recipe of tests/test_gpu_stabilize.py: _models on eight columns.  "smooth": translations of a few pixels, linear parts
    within 2 % of the identity, a6, a7 ~ N(0, 1e-4).  "wild": the same with NaN, infinities and huge finite values in any column,
    singular, mirrored and inflated linear parts, and perspective terms at and past the denominator bound, at random places."""
    rng = np.random.default_rng(2000 + npairs + (7 if kind == "wild" else 0))
    m = rng.normal(0.0, 1.0, (npairs, 8)) * _SCALE8
    if kind == "wild":
        pick = rng.random(npairs)
        col = rng.integers(0, 8, npairs)
        rows = np.arange(npairs)
        for lo, hi, value in ((0.00, 0.03, math.nan), (0.03, 0.06, math.inf), (0.06, 0.09, -math.inf), (0.09, 0.12, 1.7e308),
                              (0.12, 0.14, -1e300)):
            sel = (pick >= lo) & (pick < hi)
            m[rows[sel], col[sel]] = value
        for lo, hi, lin in ((0.14, 0.16, (-1.0, 0.0, 0.0, -1.0)),      # A = 0
                            (0.16, 0.18, (-2.0, 0.0, 0.0, 0.0)),       # a mirror, det = -1
                            (0.18, 0.20, (1.5, 0.0, 0.0, 1.0)),        # det = 5
                            (0.20, 0.22, (0.0, 1.0, 0.75, 0.0)),       # det = 0.25 exactly: usable
                            (0.22, 0.24, (1.0, 0.0, 0.0, 1.0))):       # det = 4 exactly: usable
            sel = (pick >= lo) & (pick < hi)
            m[sel, 1], m[sel, 2], m[sel, 4], m[sel, 5] = lin
        for lo, hi, a6 in ((0.24, 0.27, 0.01), (0.27, 0.30, -0.004), (0.30, 0.32, 0.0039)):   # 127.5 * |a6| = 1.28, 0.51, 0.497
            m[(pick >= lo) & (pick < hi), 6] = a6
    m.setflags(write=False)
    return m


def reach8(m, weights, w, h):
    hx, hy = stabilize.half_sides(w, h)
    return np.array([stabilize.smoothed_map8(m, f, weights, hx, hy)[1] for f in range(len(m) + 1)])


# ------------------------------------------------------------------ warps of the frame warp
NFRAMES = 11   # more frames than XCDs in one launch, with a padded last group


@functools.lru_cache(maxsize=None)
def warp_case(w, h, noc, which):
    """11 random frames and one warp each.  "a": zero, an integer translation, a half-pixel translation, a rotation by 3 degrees
    with zoom 1.1, a keystone (g6 = 0.5 / W), a warp whose denominator crosses zero inside the frame (g6 = 4 / W), a NaN warp,
    an infinite one, one that throws every sample outside, and two random small ones.  "b": two more random small ones, the
    keystone and the crossing in y (g7), a rotation with both perspective terms, NaN and infinite perspective terms, a huge
    one, an integer translation the other way, a huge negative one, and perspective terms far below one ulp of 1."""
    rng = np.random.default_rng(w * 100 + h * 10 + noc + (5000 if which == "b" else 0))
    frames = rng.integers(0, 256, (NFRAMES, h, w) + ((3,) if noc == 3 else ()), dtype=np.uint8)
    warps = np.zeros((NFRAMES, 8))
    c, s = math.cos(math.radians(3.0)) / 1.1, math.sin(math.radians(3.0)) / 1.1
    small = np.array([2.0, 0.05, 0.05, 2.0, 0.05, 0.05, 0.3 / max(w, h), 0.3 / max(w, h)])
    if which == "a":
        warps[1, [0, 3]] = 3.0, -2.0
        warps[2, [0, 3]] = 0.5, -0.5
        warps[3, :6] = 0.3, c - 1.0, -s, -0.2, s, c - 1.0
        warps[4, 6] = 0.5 / w
        warps[5, 6] = 4.0 / w
        warps[6, 2] = math.nan
        warps[7, [0, 4]] = math.inf, -math.inf
        warps[8, [0, 3]] = 3.0 * w + 5, -2.0 * h - 7
        warps[9:] = rng.normal(0.0, 1.0, (2, 8)) * small
    else:
        warps[:2] = rng.normal(0.0, 1.0, (2, 8)) * small
        warps[2, 7] = 0.5 / h
        warps[3, 7] = 4.0 / h
        warps[4] = 0.3, c - 1.0, -s, -0.2, s, c - 1.0, 0.2 / w, -0.2 / h
        warps[5, 6] = math.nan
        warps[6, 7] = math.inf
        warps[7, 6] = 1e30
        warps[8, [0, 3]] = -1.0, 1.0
        warps[9, [6, 7]] = -1e6, 3e-3
        warps[10, [6, 7]] = 1e-12, -1e-12
    for a in (frames, warps):
        a.setflags(write=False)
    return frames, warps


# ------------------------------------------------------------------ the rotating camera of the end-to-end test
def rotation_homography(pan, tilt, roll, fl):
    """K R K^-1 of a camera of focal length fl px that has rotated by the three angles (radians): a scene point at infinity seen
    at centred position x before the rotation is seen at H x after it"""
    cy, sy, cx, sx, cz, sz = math.cos(pan), math.sin(pan), math.cos(tilt), math.sin(tilt), math.cos(roll), math.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    K = np.diag([fl, fl, 1.0])
    return K @ (Rz @ Rx @ Ry) @ np.linalg.inv(K)


def model_of(H):
    """a0 .. a7 of a homography (normalised to corner entry 1): the inverse of gmotion.homography"""
    H = H / H[2, 2]
    return np.array([H[0, 2], H[0, 0] - 1, H[0, 1], H[1, 2], H[1, 0], H[1, 1] - 1, -H[2, 0], -H[2, 1]])


def apply_h(H, pts):
    q = np.c_[pts, np.ones(len(pts))] @ H.T
    return q[:, :2] / q[:, 2:]


def camera_homographies(n, fl, pan_deg, jitter_deg, seed):
    """C_0 .. C_{n-1}, C_0 = identity: every frame the camera turns by pan_deg about the vertical axis plus N(0, jitter_deg)
    (pan, tilt, roll), the angles accumulating"""
    rng = np.random.default_rng(seed)
    step = np.c_[np.full(n, math.radians(pan_deg)), np.zeros(n), np.zeros(n)]
    step = step + rng.normal(0.0, 1.0, (n, 3)) * np.radians(np.asarray(jitter_deg, np.float64))
    ang = np.cumsum(step, axis=0)
    ang[0] = 0.0
    return [rotation_homography(*ang[f], fl) for f in range(n)]


def true_models(C):
    """the models of the pairs: C_{f+1} C_f^-1 as a0 .. a7"""
    return np.array([model_of(C[f + 1] @ np.linalg.inv(C[f])) for f in range(len(C) - 1)])


def affine_part(T, w, h):
    """the least-squares affine model a0 .. a5 of the displacement field of the homography T over the w x h frame"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    xc, yc = (xs - (w - 1) / 2).ravel(), (ys - (h - 1) / 2).ravel()
    A = np.c_[np.ones_like(xc), xc, yc]
    q = apply_h(T, np.c_[xc, yc])
    return np.r_[np.linalg.lstsq(A, q[:, 0] - xc, rcond=None)[0], np.linalg.lstsq(A, q[:, 1] - yc, rcond=None)[0]]


def corners(w, h):
    hx, hy = (w - 1) / 2, (h - 1) / 2
    return np.array([[-hx, -hy], [hx, -hy], [-hx, hy], [hx, hy]])


def roughness(pos):
    """the RMS second difference of position sequences [n][k][2] over the frames"""
    d = pos[2:] - 2.0 * pos[1:-1] + pos[:-2]
    return float(np.sqrt((d * d).sum(-1).mean()))


def corner_share(warps, C, w, h, first=4, last=20):
    """The roughness left at the four frame corners, as a share of the input's, over frames first .. last (those with a full
    window).  out_f(x) = I_f(H(g_f) x) and I_f shows scene point P at C_f P, so the scene point of input corner P sits at
    inv(H(g_f)) C_f P in stabilised frame f.  warps: [n][6] or [n][8]."""
    P = corners(w, h)
    warps = np.asarray(warps, np.float64)
    g8 = np.concatenate([warps, np.zeros((len(warps), 8 - warps.shape[1]))], axis=1)
    stab = np.array([apply_h(np.linalg.inv(gmotion.homography(g8[f])) @ C[f], P) for f in range(len(C))])
    raw = np.array([apply_h(C[f], P) for f in range(len(C))])
    return roughness(stab[first:last + 1]) / roughness(raw[first:last + 1])


@functools.lru_cache(maxsize=None)
def rotating_clip(w, h, n, fl, pan_deg, jitter_deg, seed):
    """(clip [n][h][w] uint8, C): one large gen_synth texture sampled bilinearly under the homographies of camera_homographies --
    pixel x of frame f shows the texture at C_f^-1 x (centred coordinates, the texture's centre at the origin)"""
    import gen_synth
    from scipy.ndimage import map_coordinates
    C = camera_homographies(n, fl, pan_deg, jitter_deg, seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    pts = np.c_[(xs - (w - 1) / 2).ravel(), (ys - (h - 1) / 2).ravel()]
    src = [apply_h(np.linalg.inv(Cf), pts) for Cf in C]
    reach = int(math.ceil(max(np.abs(s).max(axis=0).max() for s in src))) + 2
    tw, th = 2 * reach + 1, 2 * reach + 1
    tex = gen_synth._texture(np.random.default_rng(77), th - 2 * gen_synth.MARGIN, tw - 2 * gen_synth.MARGIN)
    assert tex.shape == (th, tw)
    clip = [map_coordinates(tex, [s[:, 1] + reach, s[:, 0] + reach], order=1, mode="nearest").reshape(h, w) for s in src]
    clip = np.ascontiguousarray(np.clip(np.rint(np.stack(clip)), 0, 255).astype(np.uint8))
    clip.setflags(write=False)
    return clip, C
