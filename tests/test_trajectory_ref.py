"""CPU: the numpy statement of the temporal filter along flow trajectories (of_dis_amd/temporal.py: trajectory_filter_ref, the
definition of include/ofdis.h: ofdis_trajectory_filter, operation by operation in float32) held to the consequences the header
states.  The kernels are compared with it bit for bit in tests/test_gpu_trajfilter.py."""
import math

import numpy as np
import pytest

from of_dis_amd import tracking
from of_dis_amd.temporal import reach, temporal_filter_ref, trajectory_filter_ref, trajectory_weights
from trajfilter_cases import SIZES, coherent_case, fb_mask_ref, old_support, random_case

_f32 = np.float32


# ------------------------------------------------------------------ radius 1 is the existing filter
@pytest.mark.parametrize("alpha,beta", [(0.01, 0.5), (0.2, 3.0)])
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", [s for s in SIZES if s not in ((64, 16), (33, 7))], ids=lambda v: str(v))
@pytest.mark.parametrize("kind", ["smooth", "wild"])
def test_radius_1_matches_the_existing_filter(kind, w, h, noc, alpha, beta):
    frames, fw, rev = random_case(3, w, h, noc, kind)
    mfw, mrev = fb_mask_ref(fw, rev, alpha, beta), fb_mask_ref(rev, fw, alpha, beta)
    for wn, tau in ((1.0, math.inf), (0.5, 12.0)):
        want = temporal_filter_ref(frames, fw, rev, mfw, mrev, wn=wn, tau=tau)
        got = trajectory_filter_ref(frames, fw, rev, [wn], tau=tau, fb_check=True, alpha=alpha, beta=beta)
        assert np.array_equal(got[0], want[0]) and np.array_equal(old_support(got[1]), want[1]), (wn, tau)
        want = temporal_filter_ref(frames, fw, rev, None, None, wn=wn, tau=tau)
        got = trajectory_filter_ref(frames, fw, rev, [wn], tau=tau, fb_check=False)
        assert np.array_equal(got[0], want[0]) and np.array_equal(old_support(got[1]), want[1]), (wn, tau, "no check")


# ------------------------------------------------------------------ reach is a track
@pytest.mark.parametrize("fb_check", [False, True])
@pytest.mark.parametrize("case", ["coherent", "smooth"])
def test_forward_reach_matches_a_track(case, fb_check):
    """7 frames of 37x11: nf of every pixel of every frame is count - 1 of the track seeded there with max_steps = R"""
    n, w, h, R = 6, 37, 11, 4
    frames, fw, rev = coherent_case(n, w, h, 1) if case == "coherent" else random_case(n, w, h, 1, "smooth")
    _, support = trajectory_filter_ref(frames, fw, rev, trajectory_weights(R, 0.5), tau=math.inf, fb_check=fb_check)
    nf = reach(support)[1]
    seeds = tracking.grid_seeds(w, h, 1)
    for f in range(n + 1):
        _, counts = tracking.track_ref(fw, rev if fb_check else None, seeds, np.full(len(seeds), f), max_steps=R)
        assert np.array_equal(nf[f].ravel(), counts - 1), f
    if case == "coherent":   # walks of every length occur
        assert set(np.unique(nf[1])) == {0, 1, 2, 3, 4}


# ------------------------------------------------------------------ the two fixed points
@pytest.mark.parametrize("noc", [1, 3])
def test_zero_weights_return_the_clip(noc):
    for kind in ("smooth", "wild"):
        frames, fw, rev = random_case(3, 37, 11, noc, kind)
        for R in (1, 3, 8):
            out, support = trajectory_filter_ref(frames, fw, rev, np.zeros(R), tau=5.0)
            assert np.array_equal(out, frames) and not support.any()


@pytest.mark.parametrize("noc", [1, 3])
def test_identical_frames_with_zero_flows_return_themselves(noc):
    rng = np.random.default_rng(31 + noc)
    w, h, n = 52, 9, 6
    frames = np.repeat(rng.integers(0, 256, (1, h, w) + ((3,) if noc == 3 else ()), dtype=np.uint8), n + 1, axis=0)
    z = np.zeros((n, h, w, 2), _f32)
    for R, tau in ((1, math.inf), (3, 8.0), (8, math.inf)):
        out, support = trajectory_filter_ref(frames, z, z, trajectory_weights(R), tau=tau)
        assert np.array_equal(out, frames), (R, tau)
        nb, nf = reach(support)
        for f in range(n + 1):
            assert (nb[f] == min(R, f)).all() and (nf[f] == min(R, n - f)).all()


# ------------------------------------------------------------------ by hand
def test_two_steps_on_integer_translations():
    """five frames of 6x1, every forward flow (+1, 0) and every reverse flow (-1, 0), weights (1, 0.5), no gate: frame 2 is
    (c + I1[x-1] + I3[x+1] + 0.5 * I0[x-2] + 0.5 * I4[x+2]) / (1 + 1 + 1 + 0.5 + 0.5) over the terms whose pixel exists"""
    frames = np.array([[10, 20, 30, 40, 50, 60], [12, 24, 36, 48, 60, 72], [100, 90, 80, 70, 60, 50], [5, 15, 25, 35, 45, 55],
                       [200, 180, 160, 140, 120, 100]], np.uint8).reshape(5, 1, 6)
    fw = np.zeros((4, 1, 6, 2), _f32)
    fw[..., 0] = 1.0
    for fb_check in (False, True):
        out, support = trajectory_filter_ref(frames, fw, -fw, [1.0, 0.5], fb_check=fb_check)
        # x = 0: (100 + 15 + 80) / 2.5; 1: (90 + 12 + 25 + 70) / 3.5; 2: (80 + 24 + 35 + 5 + 60) / 4;
        # 3: (70 + 36 + 45 + 10 + 50) / 4; 4: (60 + 48 + 55 + 15) / 3.5; 5: (50 + 60 + 20) / 2.5
        assert out[2, 0].tolist() == [78, 56, 51, 53, 51, 52]
        assert support[2, 0].tolist() == [0x02, 0x12, 0x22, 0x22, 0x21, 0x20]
        assert not (support[0] >> 4).any() and not (support[4] & 15).any()
        # frame 0 walks forward only: x = 0: (10 + 24 + 0.5 * 80) / 2.5 = 29.6
        assert out[0, 0, 0] == 30 and support[0, 0, 0] == 0x02


def test_a_closed_gate_does_not_end_a_direction():
    """step 1 lands on a pixel 100 grey levels away (gate 0 at tau 10), step 2 on an equal one: it still enters"""
    frames = np.array([[50, 50, 50, 50], [0, 150, 0, 0], [0, 0, 50, 0]], np.uint8).reshape(3, 1, 4)
    fw = np.zeros((2, 1, 4, 2), _f32)
    fw[..., 0] = 1.0
    out, support = trajectory_filter_ref(frames, fw, -fw, [1.0, 1.0], tau=10.0)
    assert support[0, 0, 0] == 1 and out[0, 0, 0] == 50      # one forward step with a weight > 0: the second one
    _, inf_support = trajectory_filter_ref(frames, fw, -fw, [1.0, 1.0])
    assert inf_support[0, 0, 0] == 2


def test_weights_and_reach():
    assert trajectory_weights(3).tolist() == [1.0, 1.0, 1.0] and trajectory_weights(2, 0.25).dtype == _f32
    w = trajectory_weights(3, 0.5, sigma=2.0)
    assert w.dtype == _f32 and np.array_equal(w, (0.5 * np.exp(-np.arange(1, 4) ** 2 / 8.0)).astype(_f32))
    nb, nf = reach(np.array([0x00, 0x21, 0x88, 0x03], np.uint8))
    assert nb.tolist() == [0, 2, 8, 0] and nf.tolist() == [0, 1, 8, 3]


# ------------------------------------------------------------------ denoising with exact flows
def test_five_frames_denoise_better_than_three():
    """A smooth texture translating by (-2, -1) px per frame, 7 frames of 96x48, independent Gaussian noise of sigma 8, exact
    flows.  Mean absolute error against the clean frames on frames 2..4 cropped by 8: radius 2 (flat weights) must be at most
    0.89 of radius 1 -- halfway between sqrt(3 / 5) = 0.775 (five against three equally weighted frames) and 1."""
    w, h, n, tx, ty = 96, 48, 6, -2, -1
    Y, X = np.mgrid[0:h + n * abs(ty), 0:w + n * abs(tx)].astype(np.float64)
    T = 128 + 40 * np.sin(0.11 * X + 0.05 * Y) + 30 * np.cos(0.07 * X - 0.13 * Y) + 20 * np.sin(0.23 * Y)
    # the content of pixel p of frame k sits at p + (tx, ty) in frame k + 1
    clean = np.stack([T[-ty * k:-ty * k + h, -tx * k:-tx * k + w] for k in range(n + 1)])
    noisy = np.clip(np.rint(clean + np.random.default_rng(99).normal(0.0, 8.0, clean.shape)), 0, 255).astype(np.uint8)
    fw = np.zeros((n, h, w, 2), _f32)
    fw[..., 0], fw[..., 1] = tx, ty
    crop = (slice(2, 5), slice(8, -8), slice(8, -8))
    mae = {}
    for R in (1, 2):
        out, support = trajectory_filter_ref(noisy, fw, -fw, trajectory_weights(R))
        nb, nf = reach(support)
        assert (nb[crop] == R).all() and (nf[crop] == R).all()
        mae[R] = np.abs(out[crop].astype(np.float64) - clean[crop]).mean()
    print(f"MAE radius 1 {mae[1]:.3f}, radius 2 {mae[2]:.3f}, ratio {mae[2] / mae[1]:.3f}")
    assert mae[2] <= 0.89 * mae[1], mae
