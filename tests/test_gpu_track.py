"""-m gpu: point trajectories (include/ofdis.h: ofdis_track_points on materialised flows, ofdis_batch_track_points straight
from the level flows of a sequence context).

The standalone kernel is compared bit for bit -- tracks and counts -- with of_dis_amd/tracking.py: track_ref, the header's
definition in numpy float32; the fused kernel bit for bit with the standalone one applied to what ofdis_batch_upsample_bidir /
ofdis_batch_upsample_frames write.  Conditions on the generated inputs (enough tracks survive, tracks end in both ways) are
checked on the restatement or the standalone result, never on the kernel under test."""
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from of_dis_amd import tracking
from seq_products import INVALID, SIZE_REJECTS, assert_same_bits, flag_contexts, run_context, smooth_clip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f32 = np.float32


def assert_tracks_equal(got, want, what):
    (gt, gc), (wt, wc) = got, want
    assert gt.shape == wt.shape and gc.shape == wc.shape, (what, gt.shape, wt.shape)
    if not np.array_equal(gc, wc):
        i = int(np.flatnonzero(gc != wc)[0])
        raise AssertionError(f"{what}: {(gc != wc).sum()} of {gc.size} counts differ; first at point {i}: {gc[i]} vs {wc[i]}")
    assert_same_bits(gt, wt, what + ", tracks [frame][point][component]")


# ------------------------------------------------------------------ 1. standalone kernel against the restatement
SIZES = [(37, 11), (64, 16), (1, 9), (13, 1), (1, 1), (6, 5)]
NPAIRS = [1, 2, 5]
NPOINTS = [1, 63, 64, 65, 300]
MAX_STEPS = [0, 1, 3]


def _seed_pool(rng, w, h, n=300):
    """n seeds of every kind in a fixed shuffled order behind the centre of the image (what a case of ONE point tracks): an
    integer grid, random fractional positions, positions exactly on 0, w-1 and h-1, positions outside the image, NaN"""
    grid = tracking.grid_seeds(w, h, 1)
    grid = grid[rng.permutation(len(grid))[:100]]
    frac = np.stack([rng.uniform(0, w - 1, 120), rng.uniform(0, h - 1, 120)], 1)
    ex, ey = [0.0, w - 1.0], [0.0, h - 1.0]
    border = np.array([(x, y) for x in ex + [(w - 1) / 2, (w - 1) / 4] for y in ey] +
                      [(x, y) for x in ex for y in ey + [(h - 1) / 2, (h - 1) / 4]])
    outside = np.array([(-0.001, 0), (w - 0.999, 0), (0, -1), (0, h - 0.5), (-5, -5), (2 * w, 2 * h), (1e9, 0), (-np.inf, 0),
                        (0, np.inf), (w, h)])
    nan = np.array([(np.nan, 0), (0, np.nan), (np.nan, np.nan)])
    pool = np.concatenate([grid, frac, border, outside, nan]).astype(_f32)
    reps = -(-n // len(pool))
    centre = np.array([[(w - 1) / 2, (h - 1) / 2]], _f32)
    return np.concatenate([centre, np.concatenate([pool] * reps)[rng.permutation(len(pool) * reps)[:n - 1]]])


def _smooth_flows(w, h, npairs):
    """A constant translation that crosses about a seventh of the image over the clip plus a low-frequency perturbation of at
    most 0.05 px (none along an axis of one pixel, where any motion leaves the image); rev = -fw, so du, dv are at most 0.1
    and lhs <= 0.02 < beta."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    dx = min(1.25, 0.15 * (w - 1) / npairs)
    dy = -min(0.75, 0.15 * (h - 1) / npairs)
    fw = np.empty((npairs, h, w, 2), _f32)
    for k in range(npairs):
        fw[k, ..., 0] = dx + (0.05 if w > 1 else 0.0) * np.sin(2 * np.pi * (xs / max(w, 8) + ys / max(h, 8)) + k)
        fw[k, ..., 1] = dy + (0.05 if h > 1 else 0.0) * np.cos(2 * np.pi * (xs / max(w, 8) - ys / max(h, 8)) + 2 * k)
    return fw, -fw


def _wild_flows(rng, w, h, npairs):
    """the "wild" recipe of tests/test_gpu_interp.py (_random_case): normal flows of 3 px with large, infinite, NaN and
    image-sized values mixed in.  Along an axis of one pixel a track survives only a forward component of exactly zero, which
    the recipe never draws: there the ordinary values of the forward flow are zero, so that tracks still reach the
    inequality."""
    F = [(rng.standard_normal((npairs, h, w, 2)) * 3).astype(_f32) for _ in range(2)]
    for d, f in enumerate(F):
        pick = rng.random((npairs, h, w, 2))
        f[pick < 0.08] = (rng.standard_normal(int((pick < 0.08).sum())) * 1e4).astype(_f32)
        f[(pick >= 0.08) & (pick < 0.1)] = np.inf
        f[(pick >= 0.1) & (pick < 0.12)] = -np.inf
        f[(pick >= 0.12) & (pick < 0.14)] = np.nan
        sized = (pick >= 0.14) & (pick < 0.2)
        f[sized] = (rng.uniform(-2, 2, int(sized.sum())) * max(w, h)).astype(_f32)
        if d == 0:
            for axis, size in ((0, w), (1, h)):
                if size == 1:
                    f[..., axis][pick[..., axis] >= 0.2] = 0.0
    return F[0], F[1]


@functools.lru_cache(maxsize=None)
def _case(w, h, kind, npairs):
    rng = np.random.default_rng(1000 * w + 10 * h + npairs + (5 if kind == "wild" else 0))
    fw, rev = _smooth_flows(w, h, npairs) if kind == "smooth" else _wild_flows(rng, w, h, npairs)
    pool = _seed_pool(rng, w, h)
    seed_frames = rng.integers(-1, npairs + 2, len(pool)).astype(np.int32)  # [-1, npairs + 1]: both out-of-range values
    return fw, rev, pool, seed_frames


@pytest.mark.parametrize("kind", ["smooth", "wild"])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_standalone_matches_the_definition(gpu, w, h, kind):
    for npairs in NPAIRS:
        fw, rev, pool, seed_frames = _case(w, h, kind, npairs)
        assert {-1, npairs + 1} <= set(seed_frames.tolist())
        ends = {"outside": 0, "inconsistent": 0}
        for n, with_rev, max_steps, with_sf in itertools.product(NPOINTS, (True, False), MAX_STEPS, (False, True)):
            seeds, sf = pool[:n], seed_frames[:n] if with_sf else None
            r = rev if with_rev else None
            what = f"{w}x{h} {kind}, {npairs} pairs, {n} points, rev {with_rev}, max_steps {max_steps}, seed_frame {with_sf}"
            why = {}
            want = tracking.track_ref(fw, r, seeds, sf, max_steps, reasons=why)
            assert_tracks_equal(gpu.track_points(fw, r, seeds, sf, max_steps), want, what)
            # conditions on the inputs, from the restatement
            if kind == "smooth" and max_steps == 0:
                s0 = tracking.inside(seeds[:, 0], seeds[:, 1], w, h) & (True if sf is None else sf == 0)
                reach = (want[1][s0] == npairs + 1).sum()
                assert 2 * reach >= s0.sum(), (what, reach, s0.sum())
            if kind == "wild" and n == 300 and with_rev and max_steps == 0:
                for k in ends:
                    ends[k] += why[k]
        if kind == "wild" and npairs >= 2:
            assert ends["outside"] > 0 and ends["inconsistent"] > 0, (w, h, npairs, ends)


def test_non_default_alpha_beta(gpu):
    fw, rev, pool, seed_frames = _case(37, 11, "wild", 5)
    for alpha, beta in ((0.0, 0.0), (0.2, 3.0), (1.0, 0.25)):
        want = tracking.track_ref(fw, rev, pool, seed_frames, 0, alpha, beta)
        assert_tracks_equal(gpu.track_points(fw, rev, pool, seed_frames, 0, alpha, beta), want, f"alpha {alpha}, beta {beta}")


# ------------------------------------------------------------------ 2. every entry written once, nothing else written
@pytest.mark.parametrize("n", [1, 65, 300])
@pytest.mark.parametrize("with_counts", [True, False])
def test_every_entry_is_written_and_nothing_else(gpu, n, with_counts):
    npairs, guard = 5, 4096
    fw, rev, pool, seed_frames = _case(37, 11, "wild", npairs)
    seeds, sf = pool[:n], seed_frames[:n]
    tbytes, cbytes = (npairs + 1) * n * 8, n * 4
    dt, dc = gpu.Dev(np.full(tbytes + guard, 0xAB, np.uint8)), gpu.Dev(np.full(cbytes + guard, 0xAB, np.uint8))
    dfw, drev, ds, dsf = gpu.Dev(fw), gpu.Dev(rev), gpu.Dev(seeds), gpu.Dev(sf)
    gpu.check(gpu.lib().ofdis_track_points(dfw.ptr, drev.ptr, npairs, 37, 11, ds.ptr, dsf.ptr, n, 0, gpu.FB_ALPHA, gpu.FB_BETA,
                                           dt.ptr, dc.ptr if with_counts else None, None))
    gpu.check(gpu.lib().ofdis_sync(None))
    t, c = dt.get((tbytes + guard,), np.uint8), dc.get((cbytes + guard,), np.uint8)
    assert (t[tbytes:] == 0xAB).all() and (c[cbytes:] == 0xAB).all()
    assert not (t[:tbytes].view(np.uint32) == 0xABABABAB).any()
    if with_counts:
        assert not (c[:cbytes].view(np.uint32) == 0xABABABAB).any()
        want = tracking.track_ref(fw, rev, seeds, sf)
        assert_tracks_equal((t[:tbytes].view(_f32).reshape(npairs + 1, n, 2), c[:cbytes].view(np.int32)), want, "guarded")
    else:
        assert (c[:cbytes] == 0xAB).all()


# ------------------------------------------------------------------ 3. agreement with ofdis_fb_check
@pytest.mark.parametrize("w,h", [(37, 11), (64, 16), (6, 5)])
def test_one_step_agrees_with_fb_check(gpu, w, h):
    """integer seeds on every pixel, seed frame 0, finite flows: a track takes its first step exactly where the mask of
    ofdis_fb_check is OFDIS_FB_CONSISTENT"""
    rng = np.random.default_rng(w + h)
    # a translation small enough for the 6 x 5 image with 0.3 px of noise; the reverse flow is off by 0.8 px of noise, about
    # the size of sqrt(beta): all three codes occur at every size
    fw = (np.array([0.75, -0.5]) + rng.standard_normal((1, h, w, 2)) * 0.3).astype(_f32)
    rev = (-fw + rng.standard_normal((1, h, w, 2)) * 0.8).astype(_f32)
    mask = gpu.fb_check(fw, rev)[0]
    assert all((mask == code).any() for code in (gpu.FB_CONSISTENT, gpu.FB_INCONSISTENT, gpu.FB_OUTSIDE))
    _, counts = gpu.track_points(fw, rev, tracking.grid_seeds(w, h, 1))
    assert np.array_equal(counts.reshape(h, w) >= 2, mask == gpu.FB_CONSISTENT)


# ------------------------------------------------------------------ 4. fused kernel against the standalone one
def _clip_seeds(w, h, n):
    """(seeds, seed frames, number of leading grid seeds): a stride-5 grid at frame 0, random fractional points and border points
    with seed frames from [-1, n + 1]"""
    rng = np.random.default_rng(w + h + n)
    grid = tracking.grid_seeds(w, h, 5)
    frac = np.stack([rng.uniform(0, w - 1, 200), rng.uniform(0, h - 1, 200)], 1).astype(_f32)
    xs, ys = np.linspace(0, w - 1, 9), np.linspace(0, h - 1, 7)
    border = np.array([(x, y) for x in xs for y in (0, h - 1)] + [(x, y) for x in (0, w - 1) for y in ys], _f32)
    seeds = np.concatenate([grid, frac, border])
    sf = np.concatenate([np.zeros(len(grid), np.int32), rng.integers(-1, n + 2, len(frac) + len(border)).astype(np.int32)])
    return seeds, sf, len(grid)


# (noc, w, h, n pairs, contract, pipeline)
FUSED_CASES = [
    pytest.param(1, 256, 112, 3, 0, 1, id="gray-256x112-n3-exact"),
    pytest.param(1, 256, 112, 5, 1, 1, id="gray-256x112-n5-fused"),
    pytest.param(1, 250, 107, 5, 0, 1, id="gray-250x107-n5-exact"),
    pytest.param(1, 250, 107, 3, 1, 1, id="gray-250x107-n3-fused"),
    pytest.param(3, 256, 112, 3, 0, 1, id="rgb-256x112-n3-exact"),
    pytest.param(1, 256, 112, 5, 0, 2, id="gray-256x112-n5-exact-pipelined"),
]


@pytest.mark.parametrize("noc,w,h,n,contract,pipeline", FUSED_CASES)
def test_fused_matches_standalone_on_the_materialised_flows(gpu, noc, w, h, n, contract, pipeline):
    """the full range and the sub-range (1, n - 1), with the consistency test (against upsample_bidir's two flows) and
    without it"""
    seeds, sf, ngrid = _clip_seeds(w, h, n)
    b, _ = run_context(gpu, smooth_clip(w, h, noc, n + 1), "seq_rev", contract=contract, pipeline=pipeline)
    try:
        fused = {(first, count, fb): b.track_points(seeds, w, h, sf, fb_check=fb, first=first, count=count)
                 for first, count in ((0, n), (1, n - 1)) for fb in (True, False)}
        fused_steps = b.track_points(seeds, w, h, sf, max_steps=2)
        fw, rev, _, _ = b.upsample_bidir(w, h, outputs=(True, True, False, False))
    finally:
        b.close()
    for (first, count, fb), got in fused.items():
        sl = slice(first, first + count)
        want = gpu.track_points(fw[sl], rev[sl] if fb else None, seeds, sf)
        assert_tracks_equal(got, want, f"pairs [{first}, {first + count}), fb_check {fb}")
    assert_tracks_equal(fused_steps, gpu.track_points(fw, rev, seeds, sf, max_steps=2), "max_steps 2")
    # the clip is gentle enough for the comparison to cover whole tracks (condition on the standalone result)
    counts = gpu.track_points(fw, rev, seeds, sf)[1][:ngrid]
    assert 2 * (counts == n + 1).sum() >= ngrid, ((counts == n + 1).sum(), ngrid)


@pytest.mark.parametrize("contract", [0, 1], ids=["exact", "fused"])
def test_fused_without_the_test_on_a_forward_only_sequence(gpu, contract):
    w, h, n = 250, 107, 3
    seeds, sf, _ = _clip_seeds(w, h, n)
    b, _ = run_context(gpu, smooth_clip(w, h, 1, n + 1), "seq", contract=contract)
    try:
        got = b.track_points(seeds, w, h, sf, fb_check=False)
        fw = b.upsample_frames(0, n, w, h)
    finally:
        b.close()
    assert_tracks_equal(got, gpu.track_points(fw, None, seeds, sf), "forward-only sequence context")


# ------------------------------------------------------------------ 5. checks that need a context
@pytest.fixture(scope="module")
def contexts(gpu):
    yield from flag_contexts(gpu)


def _batch_call(gpu, b, first=0, count=3, seeds=True, tracks=True, npoints=4, max_steps=0, fb_check=1, alpha=0.01, beta=0.5,
                wo=256, ho=112):
    """host buffers stand in for the device arrays: every call returns before it would launch"""
    s, t = np.zeros((4, 2), _f32), np.zeros((4, 4, 2), _f32)
    return gpu.lib().ofdis_batch_track_points(b.h, first, count, s.ctypes.data if seeds else None, None, npoints, max_steps,
                                              fb_check, alpha, beta, t.ctypes.data if tracks else None, None, wo, ho, None)


@pytest.mark.parametrize("which", ["plain", "reverse"])
def test_batch_track_points_needs_a_sequence_context(gpu, contexts, which):
    assert _batch_call(gpu, contexts[which]) == INVALID
    assert "SEQUENCE" in gpu.lib().ofdis_last_error().decode()


def test_batch_track_points_with_the_test_needs_a_reverse_context(gpu, contexts):
    assert _batch_call(gpu, contexts["seq"], fb_check=1) == INVALID
    assert "REVERSE" in gpu.lib().ofdis_last_error().decode()


@pytest.mark.parametrize("kw", [
    dict(first=-1), dict(count=0), dict(first=1, count=3), dict(first=3, count=1), dict(count=4)] + SIZE_REJECTS + [
    dict(fb_check=2), dict(fb_check=-1), dict(seeds=False), dict(tracks=False), dict(npoints=0), dict(npoints=(1 << 24) + 1),
    dict(max_steps=-1), dict(alpha=-0.01), dict(beta=float("nan")),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_batch_track_points_rejects(gpu, contexts, kw):
    assert _batch_call(gpu, contexts["seq_rev"], **kw) == INVALID
    assert gpu.lib().ofdis_last_error()


# ------------------------------------------------------------------ the command-line tool
def test_flow_images_tracks(gpu, tmp_path):
    """tools/flow_images.py --sequence --reverse --tracks 5: <stem>_tracks.npy and <stem>_counts.npy hold what the standalone
    call makes of the .flo / .rev.flo files the same run writes; --tracks without --reverse is refused"""
    from PIL import Image
    w, h, n = 250, 107, 3
    paths = []
    for k, f in enumerate(smooth_clip(w, h, 1, n + 1)):
        paths.append(str(tmp_path / f"f{k}.png"))
        Image.fromarray(f).save(paths[-1])
    tool, stem = os.path.join(ROOT, "tools", "flow_images.py"), str(tmp_path / "clip")
    run = lambda args: subprocess.run([sys.executable, tool] + args, capture_output=True, text=True, timeout=300)
    res = run(["--sequence", "--reverse", "--tracks", "5"] + paths + [stem])
    assert res.returncode == 0, (res.stdout, res.stderr)
    read_flo = lambda path: np.fromfile(path, _f32, offset=12).reshape(h, w, 2)
    fw = np.stack([read_flo(f"{stem}_{k:03d}.flo") for k in range(n)])
    rev = np.stack([read_flo(f"{stem}_{k:03d}.rev.flo") for k in range(n)])
    tracks, counts = np.load(stem + "_tracks.npy"), np.load(stem + "_counts.npy")
    assert tracks.dtype == _f32 and counts.dtype == np.int32
    assert_tracks_equal((tracks, counts), gpu.track_points(fw, rev, tracking.grid_seeds(w, h, 5)), "the tool's files")
    res = run(["--sequence", "--tracks", "5"] + paths + [stem])
    assert res.returncode != 0 and "--reverse" in (res.stderr + res.stdout)
