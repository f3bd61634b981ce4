"""Inputs shared by tests/test_trajectory_ref.py (CPU) and tests/test_gpu_trajfilter.py: the clips and flows the trajectory filter
(include/ofdis.h: ofdis_trajectory_filter) is tested on, and the numpy statement of ofdis_fb_check's codes."""
import functools

import numpy as np

from of_dis_amd import tracking

_f32 = np.float32
SIZES = [(37, 11), (64, 16), (1, 9), (13, 1), (1, 1), (6, 5), (33, 7)]


def _frames(rng, n, w, h, noc, wild):
    shape = (n + 1, h, w) + ((3,) if noc == 3 else ())
    if wild:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    ys, xs = np.mgrid[0:h, 0:w]
    ramp = (40 + 1.5 * xs + 2.5 * ys).reshape((1, h, w) + ((1,) if noc == 3 else ()))
    return np.clip(np.rint(ramp + rng.normal(0, 2.0, shape)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def random_case(n, w, h, noc, kind):
    """npairs = n: (frames, flow_fw, flow_rev) as _random_case of tests/test_gpu_tfilter.py makes them.  "smooth" = normal flows
    of 3 px with pixels that stay put, frames a ramp plus noise of a few grey levels; "wild" = the same flows with large,
    infinite, NaN and image-sized values mixed in, frames uniform random bytes."""
    rng = np.random.default_rng(w * 1000 + h * 10 + noc + 100 * n + (5 if kind == "wild" else 0))
    frames = _frames(rng, n, w, h, noc, kind == "wild")
    F = [(rng.standard_normal((n, h, w, 2)) * 3).astype(_f32) for _ in range(2)]
    if kind == "wild":
        for f in F:
            pick = rng.random((n, h, w, 2))
            f[pick < 0.08] = (rng.standard_normal(int((pick < 0.08).sum())) * 1e4).astype(_f32)
            f[(pick >= 0.08) & (pick < 0.1)] = np.inf
            f[(pick >= 0.1) & (pick < 0.12)] = -np.inf
            f[(pick >= 0.12) & (pick < 0.14)] = np.nan
            sized = (pick >= 0.14) & (pick < 0.2)
            f[sized] = (rng.uniform(-2, 2, int(sized.sum())) * max(w, h)).astype(_f32)
    else:
        for f in F:
            f[rng.random((n, h, w)) < 0.3] = 0.0
    for a in (frames, F[0], F[1]):
        a.setflags(write=False)
    return frames, F[0], F[1]


@functools.lru_cache(maxsize=None)
def coherent_case(n, w, h, noc):
    """npairs = n: flows that pass the forward-backward test -- per pair a translation within +-1.5 px plus a ripple of 0.2 px,
    flow_rev = -flow_fw -- on the "smooth" frames: walks of several steps survive, and end at the borders."""
    rng = np.random.default_rng(7000 + w * 1000 + h * 10 + noc + 100 * n)
    frames = _frames(rng, n, w, h, noc, False)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    fw = np.empty((n, h, w, 2), _f32)
    for k in range(n):
        t = rng.uniform(-1.5, 1.5, 2)
        ph = rng.uniform(0, 2 * np.pi, 2)
        fw[k, ..., 0] = t[0] + 0.2 * np.sin(0.7 * xs + 0.4 * ys + ph[0])
        fw[k, ..., 1] = t[1] + 0.2 * np.cos(0.5 * xs - 0.6 * ys + ph[1])
    rev = -fw
    for a in (frames, fw, rev):
        a.setflags(write=False)
    return frames, fw, rev


def fb_mask_ref(flow, other, alpha, beta):
    """the codes of ofdis_fb_check(flow, other) [n][h][w] uint8 from tracking.inside / bilinear / consistent: 2 = the target is
    outside, else 0 = the inequality holds, 1 = it does not"""
    n, h, w = flow.shape[:3]
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    mask = np.empty((n, h, w), np.uint8)
    for k in range(n):
        u, v = flow[k, ..., 0].ravel(), flow[k, ..., 1].ravel()
        with np.errstate(all="ignore"):
            qx, qy = xs.ravel().astype(_f32) + u, ys.ravel().astype(_f32) + v
        ok = tracking.inside(qx, qy, w, h)
        code = np.full(h * w, 2, np.uint8)
        i = np.flatnonzero(ok)
        ru, rv = tracking.bilinear(other[k], qx[i], qy[i])
        code[i] = np.where(tracking.consistent(u[i], v[i], ru, rv, alpha, beta), 0, 1)
        mask[k] = code.reshape(h, w)
    return mask


def old_support(support):
    """the trajectory filter's support at radius 1 in the format of ofdis_temporal_filter: bit 0 here is the old bit 1 (next),
    bit 4 the old bit 0 (prev)"""
    return ((support & 1) << 1) | ((support >> 4) & 1)
