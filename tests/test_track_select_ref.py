"""CPU: the numpy model of the track selection (of_dis_amd/tracking.py: track_select_ref, the definition of include/ofdis.h:
ofdis_track_select) against hand-made tracks with known answers and against an independent float64 evaluation, and the
synthetic population tests/test_gpu_track_select.py compares the kernels on (`population`): its properties are asserted here,
on the model, never on the kernel under test."""
import functools

import numpy as np
import pytest

from of_dis_amd import tracking
from of_dis_amd.tracking import (TS_CAMERA, TS_ERRATIC, TS_INVALID, TS_JUMP, TS_KEPT, TS_SHORT, TS_STATIC, TrackSelectParams,
                                 track_select_ref)

_f32 = np.float32
SIZE = (320, 240)  # the frame the models of the population refer to


# ------------------------------------------------------------------ hand-made tracks
def _tracks(points, lmax=15):
    """a list of [L][2] point lists -> (tracks [lmax + 1][n][2] with the NaN tail of ofdis_dense_tracks, start, length)"""
    n = len(points)
    tracks = np.full((lmax + 1, n, 2), tracking.ENDED_BITS, np.uint32).view(_f32)
    length = np.zeros(n, np.int32)
    for i, p in enumerate(points):
        p = np.asarray(p, _f32).reshape(-1, 2)
        tracks[:len(p), i] = p
        length[i] = len(p)
    return tracks, np.zeros(n, np.int32), length


def _code(points, models=None, params=None, lmax=15):
    tracks, start, length = _tracks(points, lmax)
    return track_select_ref(tracks, start, length, models, SIZE if models is not None else None, params)[0]


def _walk(step, L=16, origin=(100.0, 80.0)):
    return np.asarray(origin) + np.arange(L)[:, None] * np.asarray(step, np.float64)


def _translation(u, v, npairs=15):
    m = np.zeros((npairs, 6))
    m[:, 0], m[:, 3] = u, v
    return m


def test_a_track_that_stands_still_is_static():
    assert list(_code([_walk((0, 0)), _walk((0, 0), L=1), _walk((0.1, -0.1))])) == [TS_STATIC] * 3


def test_a_straight_walk_of_one_pixel_steps_is_kept():
    """L positions one pixel apart have the spread sqrt((L^2 - 1) / 12): above sqrt(3) from L = 7 on"""
    code = _code([_walk((1, 0), L) for L in range(2, 17)])
    assert list(code) == [TS_STATIC] * 5 + [TS_KEPT] * 10
    assert _code([_walk((0, 1))])[0] == TS_KEPT and _code([_walk((0.7, -0.7))])[0] == TS_KEPT


def test_one_large_step_among_small_ones_is_a_jump():
    p = _walk((0.5, 0))
    p[8:, 0] += 30.0
    assert _code([p])[0] == TS_JUMP
    # the same step among large ones is not: 30 is below 0.7 of the path
    q = _walk((3, 0))
    q[8:, 0] += 27.0
    assert _code([q])[0] == TS_KEPT
    # ... and a step of 20 exactly is not above max_step
    r = _walk((0.5, 0))
    r[8:, 0] += 19.5
    assert _code([r])[0] == TS_KEPT


def test_a_spread_above_fifty_is_erratic():
    assert _code([_walk((12, 0))])[0] == TS_ERRATIC      # 12 * sqrt(255 / 12) = 55.3
    assert _code([_walk((0, -12))])[0] == TS_ERRATIC
    assert _code([_walk((10, 0))])[0] == TS_KEPT          # 46.1


def test_a_track_that_moves_with_the_camera():
    p = _walk((2, 1))
    m = _translation(2, 1)
    assert _code([p], m)[0] == TS_CAMERA
    assert _code([p])[0] == TS_KEPT
    assert _code([p], _translation(2, 2.5))[0] == TS_KEPT   # every residual step has the length 1.5
    # an affine model: the steps are the model's flow where the track stands
    a = np.array([1.5, 0.01, -0.02, -0.5, 0.015, 0.005])
    q = [np.array([250.0, 30.0])]
    for _ in range(15):
        xc, yc = q[-1][0] - (SIZE[0] - 1) / 2, q[-1][1] - (SIZE[1] - 1) / 2
        q.append(q[-1] + [a[0] + a[1] * xc + a[2] * yc, a[3] + a[4] * xc + a[5] * yc])
    assert _code([q], np.tile(a, (15, 1)))[0] == TS_CAMERA
    assert _code([q], _translation(0, 0))[0] == TS_KEPT


def test_a_pair_outside_the_models_is_invalid():
    tracks, start, length = _tracks([_walk((2, 1)), _walk((2, 1))])
    start[1] = 3   # its last steps are the pairs 15, 16, 17 of 15
    m = _translation(0, 0)
    assert list(track_select_ref(tracks, start, length, m, SIZE)[0]) == [TS_KEPT, TS_INVALID]
    start[1] = -1
    assert list(track_select_ref(tracks, start, length, m, SIZE)[0]) == [TS_KEPT, TS_INVALID]
    assert list(track_select_ref(tracks, start, length)[0]) == [TS_KEPT, TS_KEPT]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_position_that_is_not_finite_is_invalid(bad):
    for at in (0, 7, 15):
        for c in (0, 1):
            p = _walk((1, 1))
            p[at, c] = bad
            assert _code([p])[0] == TS_INVALID
    # beyond len it is the tail every track has
    assert _code([_walk((1, 1), L=9)])[0] == TS_KEPT


def test_len_below_min_len_is_short():
    pts = [_walk((1, 1), L) for L in (1, 8, 9, 16)]
    assert list(_code(pts, params=TrackSelectParams(min_len=9))) == [TS_SHORT, TS_SHORT, TS_KEPT, TS_KEPT]
    assert list(_code(pts, params=TrackSelectParams(min_len=17))) == [TS_SHORT] * 4
    # min_len 0 and 1 are the same test: only an empty slot is short
    tracks, start, length = _tracks(pts)
    length[1] = 0
    for min_len in (0, 1):
        assert list(track_select_ref(tracks, start, length, params=TrackSelectParams(min_len=min_len))[0]) == [TS_STATIC, TS_SHORT, TS_KEPT, TS_KEPT]
    # len above lmax + 1 counts as lmax + 1, below 0 as 0
    length[:] = [99, -5, 9, 16]
    assert list(track_select_ref(tracks, start, length)[0]) == [TS_INVALID, TS_SHORT, TS_KEPT, TS_KEPT]


def test_the_first_test_that_holds_gives_the_code():
    short_nan = _walk((1, 1), 4)
    short_nan[2, 0] = np.nan
    nan_static = _walk((0, 0))
    nan_static[3, 1] = np.inf
    erratic_jump = _walk((0.5, 0))
    erratic_jump[8:, 0] += 400.0                            # spread 200, one step of 400
    jump_camera = _walk((0.5, 0))
    jump_camera[8:, 0] += 30.0
    m = _translation(0.5, 0)
    m[7, 0] = 30.5                                          # the camera jumps with it
    static_camera = _walk((0.1, 0))
    t = TrackSelectParams(min_len=5)
    assert list(_code([short_nan, nan_static, erratic_jump, jump_camera, static_camera], m, t)) == \
        [TS_SHORT, TS_INVALID, TS_ERRATIC, TS_JUMP, TS_STATIC]
    # each falls to the next test that holds once its first is switched off
    off = lambda *codes: TrackSelectParams(min_len=5, tests=tracking.TS_ALL_TESTS & ~sum(1 << (c - 1) for c in codes))
    assert _code([short_nan], m, off(TS_SHORT))[0] == TS_INVALID
    assert _code([erratic_jump], m, off(TS_ERRATIC))[0] == TS_JUMP
    assert _code([jump_camera], m, off(TS_JUMP))[0] == TS_CAMERA
    assert _code([static_camera], _translation(0.1, 0), off(TS_STATIC))[0] == TS_CAMERA
    assert _code([nan_static], m, off(TS_INVALID))[0] == TS_KEPT   # every comparison with its NaN spread is false


def test_a_cleared_bit_skips_its_test():
    p = _walk((0.5, 0))
    p[8:, 0] += 30.0
    pts = [_walk((0, 0)), _walk((12, 0)), p, _walk((2, 1))]
    m = _translation(2, 1)
    full = _code(pts, m)
    assert list(full) == [TS_STATIC, TS_ERRATIC, TS_JUMP, TS_CAMERA]
    for i, c in enumerate(full):
        got = _code(pts, m, TrackSelectParams(tests=tracking.TS_ALL_TESTS & ~(1 << (int(c) - 1))))
        assert got[i] != c and list(np.delete(got, i)) == list(np.delete(full, i)), (c, got)
    assert not _code(pts, m, TrackSelectParams(tests=0)).any()


# ------------------------------------------------------------------ the population of the GPU test
@functools.lru_cache(maxsize=None)
def population(n, lmax, seed=2013):
    """n slots with every kind of track, in random order: (tracks [lmax + 1][n][2], start, length, translation models, affine
    models), the models float64 [npairs][6] for SIZE frames, npairs = lmax + 3.  Nobody writes to them."""
    rng = np.random.default_rng(seed + 1000 * lmax)
    npairs = lmax + 3
    tr = np.zeros((npairs, 6))
    tr[:, 0], tr[:, 3] = 5.0 + rng.uniform(-0.5, 0.5, npairs), -4.0 + rng.uniform(-0.5, 0.5, npairs)
    af = tr.copy()
    af[:, [1, 2, 4, 5]] = rng.uniform(-0.004, 0.004, (npairs, 4))
    kind = rng.choice(8, n, p=[0.34, 0.12, 0.12, 0.14, 0.08, 0.1, 0.06, 0.04])
    # 0 walker, 1 follows the translations, 2 follows the affine models, 3 static, 4 erratic, 5 jump, 6 not finite, 7 empty
    full = rng.random(n) < 0.5
    length = np.where(full, lmax + 1, rng.integers(1, lmax + 2, n))
    length[kind == 7] = 0
    length[(kind == 4) | (kind == 5) | (kind == 1) | (kind == 2)] = np.maximum(length[(kind == 4) | (kind == 5) | (kind == 1) | (kind == 2)], 2)
    start = np.array([rng.integers(0, npairs - max(L - 1, 1) + 1) for L in length])
    late = (rng.random(n) < 0.03) & (length >= 3)
    start[late] = npairs - 1                                   # their later steps have no model
    pos = np.empty((lmax + 1, n, 2))
    pos[0] = np.stack([rng.uniform(40, SIZE[0] - 40, n), rng.uniform(40, SIZE[1] - 40, n)], 1)
    angle, speed = rng.uniform(0, 2 * np.pi, n), rng.uniform(6, 10, n)
    jump_at = rng.integers(0, np.maximum(length - 1, 1))
    cx, cy = (SIZE[0] - 1) / 2, (SIZE[1] - 1) / 2
    for j in range(lmax):
        k = np.clip(start + j, 0, npairs - 1)
        step = np.stack([np.cos(angle), np.sin(angle)], 1) * speed[:, None] + rng.normal(0, 0.3, (n, 2))      # walker
        for which, m in ((1, tr), (2, af)):
            a = m[k]
            xc, yc = pos[j, :, 0] - cx, pos[j, :, 1] - cy
            flow = np.stack([a[:, 0] + a[:, 1] * xc + a[:, 2] * yc, a[:, 3] + a[:, 4] * xc + a[:, 5] * yc], 1)
            step = np.where((kind == which)[:, None], flow + rng.normal(0, 0.05, (n, 2)), step)
        step = np.where((kind == 3)[:, None], rng.normal(0, 0.2, (n, 2)), step)
        step = np.where((kind == 4)[:, None], rng.choice([-1.0, 1.0], (n, 1)) * rng.uniform(120, 200, (n, 2)), step)
        small = rng.normal(0, 0.4, (n, 2))
        small[jump_at == j] += 60.0
        step = np.where((kind == 5)[:, None], small, step)
        pos[j + 1] = pos[j] + step
    tracks = pos.astype(_f32)
    bad = np.flatnonzero(kind == 6)
    tracks[rng.integers(0, np.maximum(length[bad], 1)), bad, rng.integers(0, 2, len(bad))] = rng.choice([np.nan, np.inf, -np.inf], len(bad))
    ended = np.arange(lmax + 1)[:, None] >= length[None]
    tracks.view(np.uint32)[ended] = tracking.ENDED_BITS
    out = (tracks, start.astype(np.int32), length.astype(np.int32), tr, af)
    for a in out:
        a.setflags(write=False)
    return out


POPULATIONS = [(200, 1), (200, 2), (200, 15), (256 * 256 + 1, 2)]   # what tests/test_gpu_track_select.py takes its slots from


@pytest.mark.parametrize("n,lmax", POPULATIONS)
def test_the_population_has_every_code_and_keeps_a_fair_share(n, lmax):
    tracks, start, length, tr, af = population(n, lmax)
    assert (length == 0).any() and (length == 1).any() and (length == lmax + 1).any()
    for models, codes in ((None, range(6)), (tr, range(7)), (af, range(7))):
        code, counts = track_select_ref(tracks, start, length, models, SIZE)[:2]
        print(f"n {n} lmax {lmax} models {models is not None}: " + ", ".join(f"{k} {c}" for k, c in zip(tracking.TS_NAMES, counts)))
        assert all(counts[c] > 0 for c in codes), counts
        assert n / 5 <= counts[0] <= 4 * n / 5, counts
        assert counts.sum() == n and np.array_equal(np.bincount(code, minlength=7), counts)
        if models is None:
            assert counts[TS_CAMERA] == 0


# ------------------------------------------------------------------ the outputs
def test_counts_and_the_compacted_set():
    tracks, start, length, tr, _ = population(200, 15)
    code, counts, tracks_out, start_out, len_out, info, index, shape = track_select_ref(tracks, start, length, tr, SIZE)
    kept = np.flatnonzero(code == 0)
    assert counts.sum() == 200 and counts[0] == len(kept) and list(info) == [len(kept), 0]
    assert np.array_equal(index, kept) and index.dtype == np.int32
    assert np.array_equal(tracks_out.view(np.uint32), tracks[:, kept].view(np.uint32))         # NaN tails included
    assert np.array_equal(start_out, start[kept]) and np.array_equal(len_out, length[kept])
    assert shape.shape == (len(kept), 15, 2) and shape.dtype == _f32
    # a smaller output set: the first slots, the rest counted
    room = len(kept) // 3
    small = track_select_ref(tracks, start, length, tr, SIZE, max_out=room)
    assert list(small[5]) == [room, len(kept) - room] and np.array_equal(small[6], kept[:room])
    assert np.array_equal(small[0], code) and np.array_equal(small[1], counts)
    assert np.array_equal(small[7].view(np.uint32), shape[:room].view(np.uint32))
    # all tests off: the identity
    same = track_select_ref(tracks, start, length, tr, SIZE, TrackSelectParams(tests=0))
    assert not same[0].any() and np.array_equal(same[6], np.arange(200))
    assert np.array_equal(same[2].view(np.uint32), tracks.view(np.uint32))


def test_shape_without_models_is_the_shape_of_the_descriptors():
    """bit for bit what track_descriptors_ref returns as `shape` (its tracks have len >= 1 and stay inside their clip)"""
    tracks, start, length, _, _ = population(200, 15)
    ok = (length >= 1) & (track_select_ref(tracks, start, length)[0] != TS_INVALID)
    tracks, start, length = np.ascontiguousarray(tracks[:, ok]), np.zeros(ok.sum(), np.int32), length[ok]
    frames, flow = np.zeros((16, 4, 4), np.uint8), np.zeros((15, 4, 4, 2), _f32)   # (every window lies outside: no histogram work)
    want = tracking.track_descriptors_ref(frames, flow, tracks, start, length, 2, 1, 1, 0.0)[1]
    for t in (TrackSelectParams(tests=0), TrackSelectParams()):
        index, shape = track_select_ref(tracks, start, length, params=t)[6:]
        assert len(index) > 50 and shape.any()
        assert np.array_equal(shape.view(np.uint32), want[index].view(np.uint32))
    # with models it is the residual steps over their summed lengths: unit L1-of-norms
    tracks, start, length, tr, _ = population(200, 15)
    shape = track_select_ref(tracks, start, length, tr, SIZE)[7]
    norms = np.sqrt((shape.astype(np.float64) ** 2).sum(2)).sum(1)
    assert np.allclose(norms, 1.0, atol=1e-5)


# ------------------------------------------------------------------ an independent float64 evaluation
def _code_f64(tracks, start, length, models, t):
    """the definition written another way: whole-array float64 statistics per slot, no sequential sums"""
    lmax, n = tracks.shape[0] - 1, tracks.shape[1]
    code = np.zeros(n, np.uint8)
    for i in range(n):
        L = int(np.clip(length[i], 0, lmax + 1))
        p = tracks[:L, i].astype(np.float64)
        d = np.diff(p, axis=0)
        m = np.hypot(d[:, 0], d[:, 1])
        if L < max(t.min_len, 1):
            code[i] = TS_SHORT
        elif not np.isfinite(p).all() or (models is not None and L >= 2 and not (0 <= start[i] and start[i] + L - 2 < len(models))):
            code[i] = TS_INVALID
        elif p.std(0).max() < t.min_std:
            code[i] = TS_STATIC
        elif p.std(0).max() > t.max_std:
            code[i] = TS_ERRATIC
        elif L >= 2 and m.max() > t.max_step and m.max() > t.max_step_share * m.sum():
            code[i] = TS_JUMP
        elif models is not None and L >= 2:
            a = models[start[i]:start[i] + L - 1]
            c = p[:-1] - [(SIZE[0] - 1) / 2, (SIZE[1] - 1) / 2]
            r = d - np.stack([a[:, 0] + a[:, 1] * c[:, 0] + a[:, 2] * c[:, 1], a[:, 3] + a[:, 4] * c[:, 0] + a[:, 5] * c[:, 1]], 1)
            if np.hypot(r[:, 0], r[:, 1]).max() <= t.min_camera:
                code[i] = TS_CAMERA
    return code


@pytest.mark.parametrize("lmax", [1, 2, 15])
def test_the_model_against_float64(lmax):
    """on the slots of the population that sit far from every threshold -- those whose float64 code stays when every threshold
    moves by 5 % either way -- a float32 rounding cannot change a code, so the model must agree with the float64 evaluation"""
    tracks, start, length, tr, af = population(200, lmax)
    scaled = lambda s: TrackSelectParams(2, 2.0 * s, 55.0 * s, 30.0 * s, 0.6 * s, 0.5 * s)
    for models in (None, tr, af):
        want = _code_f64(tracks, start, length, models, scaled(1.0))
        far = np.all([_code_f64(tracks, start, length, models, scaled(s)) == want for s in (0.95, 1.05)], 0)
        assert far.mean() > 0.8 and len(np.unique(want[far])) == (6 if models is None else 7), (far.mean(), np.unique(want[far]))
        got = track_select_ref(tracks, start, length, models, SIZE, scaled(1.0))[0]
        assert np.array_equal(got[far], want[far]), models is not None
