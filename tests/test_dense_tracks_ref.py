"""CPU, numpy only: the model of the dense trajectories (of_dis_amd/tracking.py: seed_texture_ref, dense_tracks_ref) against
the consequences include/ofdis.h states -- replay through track_ref, coverage, slot order, the known count -- the texture test
against a float64 eigenvalue, and the drop policy.  The kernels are held to this model by tests/test_gpu_dense_tracks.py."""
import functools

import numpy as np
import pytest

import gen_synth
from of_dis_amd import tracking
from stereo_lr_ref import bits as _bits

_f32 = np.float32


@functools.lru_cache(maxsize=None)
def _recipe(w, h, noc, stride, window, npairs):
    """the clip of tests/test_gpu_dense_tracks.py: a texture rolled by a pixel per frame with a flat patch, a flow of about
    (1.25, -0.5) with a NaN, a reverse flow that contradicts it in the lower right quadrant; T leaves 60 % of frame 0's cells"""
    base = gen_synth.make_pair(w, h, 6200, noc)[0]
    frames = np.stack([np.roll(base, k, axis=1) for k in range(npairs + 1)])
    frames[:, :h // 3, :w // 3] = 128
    textured = lambda T: tracking.seed_texture_ref(frames[:1], stride, window, T).mean() >= 0.6
    lo, hi = 0, 2 ** 31 - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if textured(mid) else (lo, mid)
    ys, xs = np.mgrid[0:h, 0:w]
    fw = np.empty((npairs, h, w, 2), _f32)
    fw[..., 0] = (1.25 + 0.05 * np.sin(xs / 7)).astype(_f32)
    fw[..., 1] = -0.5
    rev = -fw
    rev[:, h // 2:, w // 2:] += 1.5
    fw[1, 3, 5] = np.nan
    return np.ascontiguousarray(frames), fw, rev, lo


# (w, h, noc, stride, window, npairs, max_len)
CASES = [(64, 48, 1, 2, 1, 6, 0), (64, 48, 1, 2, 1, 6, 2), (37, 11, 3, 3, 2, 5, 3), (67, 45, 1, 5, 2, 6, 4), (9, 7, 1, 4, 0, 3, 1)]
IDS = [f"{c[0]}x{c[1]}-s{c[3]}-L{c[6]}" for c in CASES]


@pytest.mark.parametrize("with_rev", [True, False], ids=["rev", "fw-only"])
@pytest.mark.parametrize("w,h,noc,stride,window,npairs,max_len", CASES, ids=IDS)
def test_replay_through_track_ref(w, h, noc, stride, window, npairs, max_len, with_rev):
    frames, fw, rev, T = _recipe(w, h, noc, stride, window, npairs)
    r = rev if with_rev else None
    tracks, start, length, info = tracking.dense_tracks_ref(frames, fw, r, stride, window, T, max_len)
    lmax = min(max_len, npairs) if max_len else npairs
    assert tracks.shape == (lmax + 1, info[0], 2) and info[0] > 0 and (start > 0).any()
    replay, counts = tracking.track_ref(fw, r, tracks[0], start, max_steps=lmax)
    assert np.array_equal(counts, length)
    assert np.array_equal(_bits(replay), _bits(tracking.to_frame_major(tracks, start, length, npairs)))
    # beyond its length a track holds the NaN pattern, inside it never a NaN
    steps = np.arange(lmax + 1)[:, None]
    assert (_bits(tracks)[steps >= length[None, :]] == tracking.ENDED_BITS).all()
    assert not np.isnan(tracks[steps < length[None, :]]).any()


@pytest.mark.parametrize("w,h,noc,stride,window,npairs,max_len", CASES, ids=IDS)
def test_coverage_and_slot_order(w, h, noc, stride, window, npairs, max_len):
    frames, fw, rev, T = _recipe(w, h, noc, stride, window, npairs)
    tracks, start, length, info = tracking.dense_tracks_ref(frames, fw, rev, stride, window, T, max_len)
    assert info[1] == 0
    lmax = tracks.shape[0] - 1
    tex = tracking.seed_texture_ref(frames, stride, window, T).reshape(npairs + 1, -1).astype(bool)
    for f in range(npairs):
        # live after step 3 of frame f: has an entry for frame f, is not complete there (a track with an entry for its last
        # frame f < npairs that ended in the step to f + 1 was still live in frame f)
        j = f - start
        live = (j >= 0) & (j < length) & (j < lmax)
        i = np.flatnonzero(live)
        cells = tracking.dense_cell(tracks[j[i], i, 0], tracks[j[i], i, 1], w, h, stride)
        covered = np.zeros(tex.shape[1], bool)
        covered[cells] = True
        assert covered[tex[f]].all(), f
    # slots are ordered by (start, cell of the seed), and no cell seeds twice in a frame
    key = start.astype(np.int64) * tex.shape[1] + tracking.dense_cell(tracks[0, :, 0], tracks[0, :, 1], w, h, stride)
    assert (np.diff(key) > 0).all()
    # every seed is a cell centre, textured in its frame
    xs, ys = tracking.dense_centres(w, h, stride)
    assert np.isin(tracks[0, :, 0], xs.astype(_f32)).all() and np.isin(tracks[0, :, 1], ys.astype(_f32)).all()
    assert tex[start, key % tex.shape[1]].all()


@pytest.mark.parametrize("npairs,max_len", [(6, 0), (6, 1), (6, 2), (6, 3), (6, 4), (6, 6), (6, 9), (5, 2), (1, 0)])
def test_known_count(npairs, max_len):
    w, h, stride = 37, 11, 3
    frames = np.stack([gen_synth.make_pair(w, h, 6200, 1)[0]] * (npairs + 1))
    zero = np.zeros((npairs, h, w, 2), _f32)
    ncx, ncy = tracking.dense_grid(w, h, stride)
    lmax = min(max_len, npairs) if max_len else npairs
    why = {}
    tracks, start, length, info = tracking.dense_tracks_ref(frames, zero, zero, stride, 2, 0, max_len, reasons=why)
    assert info.tolist() == [ncx * ncy * -(-npairs // lmax), 0]
    last = start + lmax > npairs  # the last generation when Lmax does not divide npairs
    assert (length[~last] == lmax + 1).all() and (length[last] == npairs - start[last] + 1).all()
    assert last.any() == (npairs % lmax != 0)
    assert why == dict(outside=0, inconsistent=0, complete=int((~last).sum()), reseeds=int((start > 0).sum()), dropped=0)


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h,stride,window", [(64, 48, 2, 1), (37, 11, 3, 2), (67, 45, 5, 7), (9, 7, 4, 0), (5, 2, 2, 7)])
def test_texture_test_is_the_smaller_eigenvalue(w, h, stride, window, noc):
    rng = np.random.default_rng(w * h + noc)
    a0 = gen_synth.make_pair(w, h, 6200, noc)[0]
    frames = np.stack([a0, rng.integers(0, 256, a0.shape).astype(np.uint8), np.full(a0.shape, 200, np.uint8)])
    a, b, c = tracking.structure_tensor(frames, stride, window)
    assert a.shape == (3,) + tracking.dense_grid(w, h, stride)[::-1]
    assert a.max() < 1 << 26 and c.max() < 1 << 26 and a.min() >= 0 and c.min() >= 0
    af, bf, cf = (x.astype(np.float64) for x in (a, b, c))
    lam = ((af + cf) - np.sqrt((af - cf) ** 2 + 4 * bf * bf)) / 2
    decided = 0
    for T in sorted({0, 1, 2 ** 31 - 1} | {int(t) for t in np.quantile(lam, [0.1, 0.5, 0.9])} | {int(t) + 1 for t in lam.ravel()[:8]}):
        got = tracking.seed_texture_ref(frames, stride, window, T).astype(bool)
        clear = np.abs(lam - T) >= 1e-6 * (af + cf)
        assert np.array_equal(got[clear], (lam >= T)[clear]), T
        decided += int(clear.sum())
        if T == 0:
            assert got.all()
        else:
            assert not got[2].any()  # a constant frame
    assert decided


def test_one_pixel_of_a_ramp_by_hand():
    """I = 3x + 5y: gx = 6, gy = 10 inside the image, so a window of (2wr + 1)^2 pixels has a = 36 n, b = 60 n, c = 100 n: rank
    one, lambda_min = 0"""
    ys, xs = np.mgrid[0:20, 0:20]
    frame = (3 * xs + 5 * ys).astype(np.uint8)[None]
    a, b, c = tracking.structure_tensor(frame, 6, 1)
    assert (a == 36 * 9).all() and (b == 60 * 9).all() and (c == 100 * 9).all()
    assert tracking.seed_texture_ref(frame, 6, 1, 0).all() and not tracking.seed_texture_ref(frame, 6, 1, 1).any()


def test_min_eig_from_gradient():
    assert tracking.min_eig_from_gradient(1.0, 2, 3) == 4 * 25 * 3
    assert tracking.min_eig_from_gradient(0.001, 0, 1) == 1 and tracking.min_eig_from_gradient(0.0, 7, 3) == 0
    assert tracking.min_eig_from_gradient(1e30, 7, 3) == 2 ** 31 - 1


@pytest.mark.parametrize("w,h,noc,stride,window,npairs,max_len", CASES[:4], ids=IDS[:4])
def test_drop_policy(w, h, noc, stride, window, npairs, max_len):
    frames, fw, rev, T = _recipe(w, h, noc, stride, window, npairs)
    full = tracking.dense_tracks_ref(frames, fw, rev, stride, window, T, max_len)
    n = int(full[3][0])
    why = {}
    tracks, start, length, info = tracking.dense_tracks_ref(frames, fw, rev, stride, window, T, max_len, max_tracks=n // 2, reasons=why)
    assert info[0] == n // 2 and info[1] > 0 and why["dropped"] == info[1]
    assert tracks.shape[1] == n // 2
    # the walks do not depend on each other and the slots are numbered in (start, cell) order: up to the frame where the cap
    # bites the two runs are one, in that frame the capped run takes the first of the uncapped run's seeds, later none -- its
    # slots are the first n // 2 of the uncapped run, bit for bit
    assert np.array_equal(start, full[1][:n // 2]) and np.array_equal(length, full[2][:n // 2])
    assert np.array_equal(_bits(tracks), _bits(full[0][:, :n // 2]))
    assert info[1] >= n - n // 2  # (a dropped seed leaves its cell unoccupied: it is dropped again in the next frame)
    # ample room changes nothing
    again = tracking.dense_tracks_ref(frames, fw, rev, stride, window, T, max_len, max_tracks=n)
    assert all(np.array_equal(_bits(x) if x.dtype == _f32 else x, _bits(y) if y.dtype == _f32 else y) for x, y in zip(again, full))
