"""-m gpu: trajectory-aligned descriptors (include/ofdis.h: ofdis_track_descriptors).

hist is compared as integers and shape as fp32 bits with of_dis_amd/tracking.py (track_descriptors_ref: the header's definition
in numpy).  Conditions on the generated inputs (every bin is voted for, windows are cut by the border, tracks of length 1 and
complete tracks exist, values are clamped and skipped) are checked on the model, never on the kernel under test.

What the model gave for the gray cases when the recipe was written (tracks, of length 1, complete, windows cut, largest entry):
64x48 N 16: 1764, 773, 685, 1051, 149839; 37x11 N 8: 103, 51, 20, 56, 107276 (RGB: 109, 58, 19, 49); 67x45 N 32: 247, 119, 63,
296, 635206; 64x48 N 64: every one of the 2524 windows cut, 926164.  The cases with other cell sides and more temporal cells (tracks, of
length 1, complete): 64x48 stride 4 N 10 nt 8 of 8: 467, 264, 67; 37x11 N 6 nt 5 of 7: 122, 65, 7; 67x45 N 18: 247, 119, 63; 64x48
stride 4 N 20: 432, 195, 159; every temporal cell of each is voted into.  Indicative only: the libm behind sin may move a last digit."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gen_synth
from of_dis_amd import tracking
from seq_products import run_context, smooth_clip
from test_gpu_dense_tracks import STRIDE, WINDOW, _clip_threshold, _threshold, _wild_flows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f32 = np.float32
MIN_FLOW = 0.4
GUARD = 4096


def assert_descriptors_equal(got, want, what):
    """(hist, shape) of two runs: hist as integers, shape as fp32 bits (shape None on both sides or on neither)"""
    (gh, gs), (wh, ws) = got, want
    assert gh.dtype == wh.dtype == np.uint32 and gh.shape == wh.shape, (what, gh.dtype, gh.shape, wh.shape)
    if not np.array_equal(gh, wh):
        bad = np.argwhere(gh != wh)
        i, e = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {gh.size} hist entries differ; first at slot {i}, entry {e}: {gh[i, e]} vs {wh[i, e]}")
    assert (gs is None) == (ws is None), what
    if gs is not None:
        assert gs.dtype == ws.dtype == _f32 and gs.shape == ws.shape, (what, gs.shape, ws.shape)
        g, w = gs.view(np.uint32), ws.view(np.uint32)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            i, j, c = bad[0]
            raise AssertionError(f"{what}: {len(bad)} of {g.size} shape values differ; first at slot {i}, step {j}, component {c}: "
                                 f"{gs[i, j, c]!r} vs {ws[i, j, c]!r}")


# ------------------------------------------------------------------ the recipe
@functools.lru_cache(maxsize=None)
def _frames(w, h, noc, stride, window, npairs):
    """the frames of tests/test_gpu_dense_tracks.py: one texture rolled by a pixel per frame, the upper-left third flat; T: the
    largest threshold that leaves 60 % of frame 0's cells textured"""
    base = gen_synth.make_pair(w, h, 6200, noc)[0]
    frames = np.stack([np.roll(base, k, axis=1) for k in range(npairs + 1)])
    frames[:, :h // 3, :w // 3] = 128
    return np.ascontiguousarray(frames), _threshold(frames[0], stride, window, 0.6)


@functools.lru_cache(maxsize=None)
def _flows(w, h, npairs):
    """a flow that turns with the position and the pair (every octant of HOF and of both MBH channels), a slow block in the
    middle (HOF's ninth bin), one NaN; a reverse flow that contradicts it in the lower-right quadrant"""
    ys, xs = np.mgrid[0:h, 0:w]
    fw = np.empty((npairs, h, w, 2), _f32)
    for k in range(npairs):
        fw[k, ..., 0] = (1.5 * np.sin(ys / 5 + 0.7 * k) + 0.4 * np.cos(xs / 3)).astype(_f32)
        fw[k, ..., 1] = (1.5 * np.cos(xs / 6 - 0.5 * k) + 0.4 * np.sin(ys / 4)).astype(_f32)
    fw[:, h // 2 - 4:h // 2 + 4, w // 2 - 6:w // 2 + 6] *= _f32(0.1)
    fw[1, 3, 5] = np.nan
    rev = -fw
    rev[:, h // 2:, w // 2:] += 1.5
    return fw, rev


@functools.lru_cache(maxsize=None)
def _case(w, h, stride, window, npairs, max_len, N, nxy, nt, noc, capacity=None):
    """inputs, tracks of the numpy model and the model's descriptors of them, computed once and shared (nobody writes to them)"""
    frames, T = _frames(w, h, noc, stride, window, npairs)
    fw, rev = _flows(w, h, npairs)
    tracks, start, length, info = tracking.dense_tracks_ref(frames, fw, rev, stride, window, T, max_len, max_tracks=capacity)
    stats = {}
    want = tracking.track_descriptors_ref(frames, fw, tracks, start, length, N, nxy, nt, MIN_FLOW, stats=stats)
    for a in (frames, fw, tracks, start, length, info) + want:
        a.setflags(write=False)
    return frames, fw, (tracks, start, length, info), want, stats


# (w, h, stride, window, npairs, max_len, N, nxy, nt)
CASES = [(64, 48, 2, 1, 6, 3, 16, 2, 3), (37, 11, 3, 2, 5, 3, 8, 2, 2), (67, 45, 5, 2, 6, 4, 32, 2, 2), (9, 7, 4, 0, 3, 2, 8, 2, 1),
         (64, 48, 2, 1, 6, 3, 64, 4, 1),
         # cell sides that are no power of two (the reciprocal of the cell side), every lane in one cell (nxy 1), nt > 3:
         # nxy 1 with a side of 10 and nt = lmax = 8; nxy 2 with a side of 3 and nt 5 in lmax 7 (temporal cells of 1 and 2 steps);
         # nxy 3 with a side of 6 and nt 3 in lmax 4; nxy 4 with a side of 5
         (64, 48, 4, 1, 8, 8, 10, 1, 8), (37, 11, 3, 2, 7, 7, 6, 2, 5), (67, 45, 5, 2, 6, 4, 18, 3, 3), (64, 48, 4, 1, 6, 3, 20, 4, 2)]
IDS = [f"{c[0]}x{c[1]}-s{c[2]}-L{c[5]}-N{c[6]}-{c[7]}x{c[7]}x{c[8]}" for c in CASES]


# ------------------------------------------------------------------ 1. against the definition
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_descriptors_match_the_definition(gpu, case, noc):
    w, h, _, _, npairs, max_len, N, nxy, nt = case
    frames, fw, (tracks, start, length, info), want, stats = _case(*case, noc)
    # conditions on the inputs, from the model
    lmax = tracks.shape[0] - 1
    assert lmax == min(max_len, npairs) and info[0] == len(length) > 0 and info[1] == 0
    if (w, h) != (9, 7):
        layout = tracking.descriptor_layout(N, nxy, nt)
        total = want[0].astype(np.int64).sum(0)
        for name, (off, bins) in layout["channels"].items():
            per_bin = total[off:off + bins * nt * nxy * nxy].reshape(-1, bins).sum(0)
            assert (per_bin > 0).all(), (name, per_bin)
        assert stats["cut"] > 0 and (length == 1).sum() > 0 and (length == lmax + 1).sum() > 0, (stats, np.bincount(length))
    print(f"{w}x{h} noc {noc} N {N}: {len(length)} tracks, {(length == 1).sum()} of length 1, {(length == lmax + 1).sum()} complete, "
          f"{stats['cut']} of {stats['windows']} windows cut, largest entry {want[0].max(initial=0)}")
    assert_descriptors_equal(gpu.track_descriptors(frames, fw, tracks, start, length, N, nxy, nt, MIN_FLOW), want, "with shape")
    assert_descriptors_equal(gpu.track_descriptors(frames, fw, tracks, start, length, N, nxy, nt, MIN_FLOW, shape=False),
                             (want[0], None), "shape NULL")


# ------------------------------------------------------------------ 2. wild flows
def test_descriptors_on_wild_flows(gpu):
    """flows with large, infinite, NaN and image-sized values: values are clamped to 65535, pixels are skipped"""
    w, h, npairs, stride, window, max_len = 37, 11, 5, 3, 2, 3
    frames, T = _frames(w, h, 1, stride, window, npairs)
    fw, rev = _wild_flows(np.random.default_rng(3711), w, h, npairs)
    for r in (rev, None):
        tracks, start, length, _ = tracking.dense_tracks_ref(frames, fw, r, stride, window, T, max_len)
        for N, nxy, nt, min_flow in ((8, 2, 2, MIN_FLOW), (12, 3, 3, 0.0)):
            stats = {}
            want = tracking.track_descriptors_ref(frames, fw, tracks, start, length, N, nxy, nt, min_flow, stats=stats)
            assert stats["clamped"] > 0 and stats["skipped"] > 0 and (length > 1).sum() > 0, stats
            assert want[0].max() >= 65535
            assert_descriptors_equal(gpu.track_descriptors(frames, fw, tracks, start, length, N, nxy, nt, min_flow), want,
                                     f"wild, N {N}, rev {r is not None}")


# ------------------------------------------------------------------ 3. every entry written, nothing else written
@pytest.mark.parametrize("with_shape", [True, False])
@pytest.mark.parametrize("capped", [False, True])
def test_every_entry_is_written_and_nothing_else(gpu, capped, with_shape):
    case = CASES[0]
    w, h, _, _, npairs, _, N, nxy, nt = case
    full = len(_case(*case, 1)[2][1])
    frames, fw, (tracks, start, length, info), want, _ = _case(*case, 1, capacity=full // 2 if capped else None)
    n, lmax = len(length), tracks.shape[0] - 1
    assert info[0] == n and (info[1] > 0) == capped
    max_tracks = n if capped else n + 100   # (a capped run of ofdis_dense_tracks fills its arrays)
    D = tracking.descriptor_layout(N, nxy, nt)["dims"]
    # the arrays of ofdis_dense_tracks with max_tracks slots: 0xAB in the slots it did not write
    padded = lambda a, shape: np.concatenate([a, np.full(shape, 0xAB, np.uint8).view(a.dtype)], axis=a.ndim - 2 if a.ndim > 1 else 0)
    spare = max_tracks - n
    dt = gpu.Dev(padded(tracks, (lmax + 1, spare, 8)) if spare else tracks)
    ds, dl = (gpu.Dev(padded(a, (spare * 4,)) if spare else a) for a in (start, length))
    di, dfr, dfw = gpu.Dev(info), gpu.Dev(frames), gpu.Dev(fw)
    sizes = dict(hist=max_tracks * D * 4, shape=max_tracks * lmax * 8)
    dev = {k: gpu.Dev(np.full(v + GUARD, 0xAB, np.uint8)) for k, v in sizes.items()}
    gpu.track_descriptors_dev(dfr.ptr, dfw.ptr, npairs, w, h, 1, dt.ptr, ds.ptr, dl.ptr, di.ptr, lmax, max_tracks, N, nxy, nt, MIN_FLOW,
                              dev["hist"].ptr, dev["shape"].ptr if with_shape else None)
    gpu.check(gpu.lib().ofdis_sync(None))
    raw = {k: dev[k].get((v + GUARD,), np.uint8) for k, v in sizes.items()}
    for k, v in sizes.items():
        assert (raw[k][v:] == 0xAB).all(), f"guard behind {k}"
    hist = raw["hist"][:sizes["hist"]].view(np.uint32).reshape(max_tracks, D)
    shape = raw["shape"][:sizes["shape"]].view(np.uint32).reshape(max_tracks, lmax, 2)
    assert (hist[n:] == 0xABABABAB).all() and (shape[n:] == 0xABABABAB).all()
    # no entry of the model is 0xABABABAB (hist below 2^32 by far, shape within [-1, 1]), so a kept fill is an unwritten entry
    assert want[0].max() < 0xABABABAB
    assert not (hist[:n] == 0xABABABAB).any()
    if with_shape:
        assert not (shape[:n] == 0xABABABAB).any()
        assert_descriptors_equal((hist[:n], shape[:n].view(_f32)), want, "guarded")
    else:
        assert (shape == 0xABABABAB).all()
        assert np.array_equal(hist[:n], want[0])
    # the inputs are inputs
    assert np.array_equal(di.get((2,), np.int64), info) and np.array_equal(dl.get((max_tracks,), np.int32)[:n], length)


# ------------------------------------------------------------------ 4. known value
def test_known_value_on_the_device(gpu):
    """zero flows, T = 0: every track stands on its cell centre; all of HOF in bin 8, 256 per pixel inside the image and step"""
    w, h, npairs, stride, max_len, N, nxy, nt = 37, 11, 5, 3, 3, 8, 2, 2
    frames, _ = _frames(w, h, 1, stride, 2, npairs)
    zero = np.zeros((npairs, h, w, 2), _f32)
    tracks, start, length, _ = tracking.dense_tracks_ref(frames, zero, zero, stride, 2, 0, max_len)
    assert (length == max_len + 1).any() and (length < max_len + 1).any()
    hist, shape = gpu.track_descriptors(frames, zero, tracks, start, length, N, nxy, nt, MIN_FLOW)
    layout = tracking.descriptor_layout(N, nxy, nt)
    chan = lambda name: hist[:, layout["channels"][name][0]:][:, :layout["channels"][name][1] * nt * nxy * nxy]
    assert not chan("mbhx").any() and not chan("mbhy").any() and not shape.any()
    hof = chan("hof").reshape(-1, nt, nxy, nxy, 9)
    assert not hof[..., :8].any()
    cs = N // nxy
    lo = lambda centre, c: centre - N // 2 + c * cs
    inside = lambda centre, c, size: np.clip(np.minimum(lo(centre, c) + cs, size) - np.maximum(lo(centre, c), 0), 0, cs)
    cx, cy = tracks[0, :, 0].astype(np.int64), tracks[0, :, 1].astype(np.int64)
    steps = np.stack([sum((j * nt // max_len == t) & (length - 1 > j) for j in range(max_len)) for t in range(nt)], 1)  # [n][nt]
    for r in range(nxy):
        for c in range(nxy):
            want = 256 * (inside(cx, c, w) * inside(cy, r, h))[:, None] * steps
            assert np.array_equal(hof[:, :, r, c, 8], want), (r, c)
    assert_descriptors_equal((hist, shape), tracking.track_descriptors_ref(frames, zero, tracks, start, length, N, nxy, nt, MIN_FLOW),
                             "known value")
    # a constant clip: no HOG either
    flat = np.full_like(frames, 91)
    hist, _ = gpu.track_descriptors(flat, zero, tracks, start, length, N, nxy, nt, MIN_FLOW)
    assert not hist[:, :layout["channels"]["hof"][0]].any() and hist.any()


# ------------------------------------------------------------------ 5. end to end through a sequence context
@pytest.mark.parametrize("contract", [0, 1], ids=["exact", "fused"])
def test_end_to_end_through_a_sequence_context(gpu, contract):
    """upsample_bidir -> dense_tracks -> track_descriptors, all on the device, against the model on the same arrays"""
    w, h, n, N, nxy, nt = 250, 107, 3, 16, 2, 3
    frames = smooth_clip(w, h, 1, n + 1)
    T = _clip_threshold(frames, STRIDE, WINDOW)
    b, _ = run_context(gpu, frames, "seq_rev", contract=contract)
    try:
        fw, rev, _, _ = b.upsample_bidir(w, h, outputs=(True, True, False, False))
    finally:
        b.close()
    tracks, start, length, info = gpu.dense_tracks(frames, fw, rev, STRIDE, WINDOW, T, n)
    assert info[0] > 0 and (length > 1).sum() > 0 and (length == n + 1).sum() > 0
    stats = {}
    want = tracking.track_descriptors_ref(frames, fw, tracks, start, length, N, nxy, nt, MIN_FLOW, stats=stats)
    assert stats["cut"] > 0 and want[0].any()
    assert_descriptors_equal(gpu.track_descriptors(frames, fw, tracks, start, length, N, nxy, nt, MIN_FLOW), want, "sequence context")


# ------------------------------------------------------------------ 6. the command-line tool
def test_flow_images_descriptors(gpu, tmp_path):
    """tools/flow_images.py --sequence --reverse --dense-tracks 5:2:T:3 --descriptors 16:2:3:0.4: <stem>_dhist.npy and
    _dshape.npy hold what the standalone call makes of the .flo files and the track files the same run writes; without
    --dense-tracks it is refused"""
    from PIL import Image
    w, h, n = 250, 107, 3
    frames = smooth_clip(w, h, 1, n + 1)
    T = _clip_threshold(frames, STRIDE, WINDOW)
    paths = []
    for k, f in enumerate(frames):
        paths.append(str(tmp_path / f"f{k}.png"))
        Image.fromarray(f).save(paths[-1])
    tool, stem = os.path.join(ROOT, "tools", "flow_images.py"), str(tmp_path / "clip")
    run = lambda args: subprocess.run([sys.executable, tool] + args, capture_output=True, text=True, timeout=300)
    res = run(["--sequence", "--reverse", "--dense-tracks", f"5:2:{T}:3", "--descriptors", "16:2:3:0.4"] + paths + [stem])
    assert res.returncode == 0, (res.stdout, res.stderr)
    fw = np.stack([np.fromfile(f"{stem}_{k:03d}.flo", _f32, offset=12).reshape(h, w, 2) for k in range(n)])
    tracks, start, length, hist, shape = (np.load(stem + f"_{name}.npy") for name in ("dtracks", "dstart", "dlen", "dhist", "dshape"))
    assert hist.dtype == np.uint32 and shape.dtype == _f32 and hist.shape == (len(length), 33 * 4 * 3) and hist.any()
    assert_descriptors_equal((hist, shape), gpu.track_descriptors(frames, fw, tracks, start, length, 16, 2, 3, 0.4), "the tool's files")
    res = run(["--sequence", "--reverse", "--descriptors", "16:2:3:0.4"] + paths + [stem])
    assert res.returncode != 0 and "--dense-tracks" in (res.stderr + res.stdout)
