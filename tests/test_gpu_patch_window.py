"""GPU: the gray 8x8 patch kernel keeps its 9 x 3 tap window in registers between evaluations and loads it again only when
the window's integer position has moved (ofdis_tuning.patch_window_reuse, fused contract).  The registers hold what a reload
would return, so the results must not depend on the knob: p and the dense flow of one level, bit for bit, with the knob on
and off, on inputs chosen for what the window does on them (CASES).  The per-level entry does not return pweight; it is
observed through the dense flow, every pixel of which is a sum over its covering patches weighted by 1 / max(|pweight|, 2)
(the inputs carry pixel noise so that the weights lie on both sides of that floor).

Geometry: one level of 120 x 60 pixels, 30 x 15 = 450 patches (28 full wavefronts of 16 patches and one of two, whose idle
lane groups shadow the last patch), two frames per launch: the pair and the pair reversed.

Under the exact contract the kernel reloads in every evaluation whatever the knob says (the window would cost it its fourth
wavefront per SIMD); there the results must stay bit-identical to the oracle."""
import functools

import numpy as np
import pytest
from scipy.ndimage import gaussian_filter, map_coordinates

import oracle
from common import assert_bits_equal
from of_dis_amd.params import oppoint

W, H = 120, 60
CASES = ("subpixel", "several_pixels", "straddle", "reset_oob", "warm_start")
_f32 = np.float32


def _params():
    p = oppoint(2, W, H).copy(sc_f=1, sc_l=0)
    p.width, p.height = W, H
    return p


def _pair(seed, u, v, noise):
    """Frame A = a band-limited texture, frame B = the texture moved by the flow (u, v) (arrays or constants), both with
    their own pixel noise of `noise` grey levels."""
    rng = np.random.default_rng(seed)
    m = 16
    tex = np.zeros((H + 2 * m, W + 2 * m))
    for sigma, amp in ((1.2, 1.0), (3.0, 1.5), (8.0, 2.0)):  # (structure at the scale of an 8 x 8 patch, as a pyramid level has it)
        tex += amp * sigma * gaussian_filter(rng.standard_normal(tex.shape), sigma, mode="wrap")
    tex = (tex - tex.mean()) / tex.std() * 45.0 + 128.0
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    a = tex[m:m + H, m:m + W]
    b = map_coordinates(tex, [yy - v + m, xx - u + m], order=3, mode="nearest")
    out = [np.clip(np.rint(x + rng.normal(0, noise, (H, W))), 0, 255).astype(np.uint8) for x in (a, b)]
    return out[0], out[1]


def patch_starts(p, level, flow_prev):
    """Reference points (rx, ry) and start displacements p_in of the level's patches in the order of the results
    (ip = gx * noph + gy; patchgrid.cpp:42-48, 62-69, 195-211)."""
    w, h = p.level_size(level)
    s = p.steps
    nw, nh = p.grid(level)
    offw, offh = (w - (nw - 1) * s) // 2, (h - (nh - 1) * s) // 2
    gx, gy = np.repeat(np.arange(nw), nh), np.tile(np.arange(nh), nw)
    rx, ry = gx * s + offw, gy * s + offh
    pin = np.zeros((nw * nh, 2), _f32)
    if flow_prev is not None:
        pin = (flow_prev[ry // 2, rx // 2] * _f32(2)).astype(_f32)
    return rx, ry, pin


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (params, planes [A, A_dx, A_dy, B] each [2, tmp_h, tmp_w, 1] of level 0, flow_prev [2, H/2, W/2, 2] or None)"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    prev = None
    if name == "subpixel":        # the search stays inside one pixel: the window of the first evaluation serves all 13
        ia, ib = _pair(11, 0.4, 0.5, 1.5)
    elif name == "several_pixels":  # 1 .. 3.5 px from a zero start, varying over the grid: patches of one wavefront cross
        u = 1.9 + 1.1 * np.sin(2 * np.pi * 1.3 * xx / W + 0.5)  # their pixel borders in different iterations
        v = -1.5 + 1.0 * np.cos(2 * np.pi * 0.9 * yy / H)
        ia, ib = _pair(12, u, v, 1.5)
    elif name == "straddle":      # converges onto an integer position: pos0 / pos1 flip between evaluations
        ia, ib = _pair(13, 1.0, -2.0, 1.5)
    elif name == "reset_oob":     # motion beyond the outlier threshold (P/2 = 4 px) in the right half; a start from a
        u = np.where(xx > W / 2, 7.5, 1.2)  # coarser flow that throws the leftmost patches out of the image
        ia, ib = _pair(14, u, -0.7, 1.5)
        prev = np.zeros((H // 2, W // 2, 2), _f32)
        prev[:, :6, 0] = -30.0
        prev[: H // 4, 6:12, 1] = -25.0
    elif name == "warm_start":    # 4 .. 8 px: found from the coarser level's flow, out of reach from zero
        u = 5.8 + 1.7 * np.sin(2 * np.pi * 0.8 * yy / H + 0.2)
        v = -3.1 + 1.2 * np.cos(2 * np.pi * 1.1 * xx / W)
        ia, ib = _pair(15, u, v, 1.5)
    else:
        raise KeyError(name)
    p = _params()
    O = oracle.c_oracle()
    O.set_reduce_order(True)
    fw, bw = O.build_pyramid(p, ia), O.build_pyramid(p, ib)
    if name == "warm_start":
        prev = O.patchgrid_level(p, 1, fw[0][1], fw[1][1], fw[2][1], bw[0][1], None)[1]
    planes = [np.stack([fw[k][0], bw[k][0]]) for k in range(3)] + [np.stack([bw[0][0], fw[0][0]])]
    prev2 = None if prev is None else np.stack([prev, prev])
    return p, planes, prev2


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's (p, dense flow, pweight) of the case's two frames."""
    p, planes, prev = case(name)
    O = oracle.c_oracle()
    O.set_reduce_order(True)
    return [O.patchgrid_level(p, 0, *[pl[f] for pl in planes], None if prev is None else prev[f], want_pweight=True)
            for f in range(2)]


def _run(gpu, name, contract, reuse):
    p, planes, prev = case(name)
    old = gpu.set_tuning(contract=contract, patch_window_reuse=reuse)
    try:
        return gpu.patchgrid_level(p, 0, *planes, prev)
    finally:
        gpu.restore_tuning(old)


def test_geometry_leaves_a_partial_wavefront():
    p = _params()
    nw, nh = p.grid(0)
    assert (W, H) == p.level_size(0) and W <= 128 and H <= 64 and (nw * nh) % 16 != 0, (nw, nh)


def test_the_inputs_do_what_they_are_named_for():
    """Conditions on the inputs, on the oracle's results (frame 0)."""
    within = {}
    for name in CASES:
        p, _, prev = case(name)
        rp, _, rpw = reference(name)[0]
        _, _, pin = patch_starts(p, 0, None if prev is None else prev[0])
        within[name] = rp - pin
        written = rpw[(rpw != 0).any(1)]   # the dense flow shows a weight where it is above the densification's floor of 2
        assert 0.3 < (written > 2).mean() < 0.8, (name, (written > 2).mean())
        if name == "reset_oob":
            # p == p_in: the patch never left its start.  Out of bounds at the start: no evaluation, the weights keep their
            # zeros; outlier reset: the evaluation after the reset wrote them
            stay = (rp == pin).all(1)
            unwritten = (rpw == 0).all(1)
            assert (stay & unwritten).sum() >= 8 and (stay & ~unwritten).sum() >= 8, ((stay & unwritten).sum(), (stay & ~unwritten).sum())
            assert (~stay).sum() >= 100
    d = within["subpixel"]
    assert ((d > 0.05) & (d < 0.95)).all(1).mean() > 0.9            # one pixel cell, start included (pos = ceil(x + 1e-5))
    d = within["several_pixels"]
    assert (np.abs(d).max(1) > 1.0).mean() > 0.8 and np.ptp(np.floor(d[:, 0])) >= 2
    d = within["straddle"] - np.array([1.0, -2.0], _f32)
    assert (np.abs(d) < 0.05).all(1).mean() > 0.5 and (d[:, 0] > 0).any() and (d[:, 0] < 0).any()
    p, _, prev = case("warm_start")
    _, _, pin = patch_starts(p, 0, prev[0])
    assert np.median(np.hypot(pin[:, 0], pin[:, 1])) > 4.0            # beyond the outlier threshold of a zero start


@pytest.mark.gpu
@pytest.mark.parametrize("contract", ["fused", "exact"])
@pytest.mark.parametrize("name", CASES)
def test_reuse_changes_no_bit(gpu, name, contract):
    c = 1 if contract == "fused" else 0
    on = _run(gpu, name, c, 1)
    off = _run(gpu, name, c, 0)
    assert_bits_equal(on[0], off[0], f"{name}, {contract} contract: patch displacements, reuse on against off")
    assert_bits_equal(on[1], off[1], f"{name}, {contract} contract: dense flow (p and pweight), reuse on against off")
    assert np.abs(on[0]).max() > 0.3  # (a search took place)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_exact_contract_stays_on_the_oracle(gpu, name):
    got = _run(gpu, name, 0, 1)
    want = reference(name)
    for f in range(2):
        assert_bits_equal(got[0][f], want[f][0], f"{name} frame {f}: patch displacements")
        assert_bits_equal(got[1][f], want[f][1], f"{name} frame {f}: dense flow")
