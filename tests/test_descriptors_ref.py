"""CPU: the numpy model of the track descriptors (of_dis_amd/tracking.py: track_descriptors_ref, descriptor_layout,
normalize_descriptors) against the consequences include/ofdis.h states, a case computed by hand and a rotation of the whole
input.  The kernel is compared with this model bit for bit in tests/test_gpu_descriptors.py."""
import numpy as np
import pytest

from of_dis_amd import tracking

_f32 = np.float32


def _channel(hist, layout, name):
    """[ntracks][nt][cell row][cell column][bin] of a channel"""
    off, bins = layout["channels"][name]
    nt, ny, nx = layout["cells"]
    return hist[:, off:off + bins * nt * ny * nx].reshape(-1, nt, ny, nx, bins)


def _still_tracks(centres, start, length, lmax):
    """tracks that stand still at the given centres"""
    centres = np.asarray(centres, _f32)
    tracks = np.full((lmax + 1, len(centres), 2), tracking.ENDED_BITS, np.uint32).view(_f32)
    for i, n in enumerate(length):
        tracks[:n, i] = centres[i]
    return tracks, np.asarray(start, np.int32), np.asarray(length, np.int32)


# ------------------------------------------------------------------ known value
def test_zero_flow_puts_hof_in_the_still_bin_and_leaves_mbh_empty():
    w, h, npairs, lmax, N, nxy, nt = 20, 14, 5, 4, 8, 2, 3
    rng = np.random.default_rng(1)
    frames = rng.integers(0, 256, (npairs + 1, h, w), dtype=np.uint8)
    centres = [(10, 7), (1, 1), (19, 13), (0, 6), (10, 0)]
    tracks, start, length = _still_tracks(centres, [0, 1, 0, 2, 0], [5, 5, 3, 1, 2], lmax)
    stats = {}
    hist, shape = tracking.track_descriptors_ref(frames, np.zeros((npairs, h, w, 2), _f32), tracks, start, length, N, nxy, nt, 0.4,
                                                 stats=stats)
    layout = tracking.descriptor_layout(N, nxy, nt)
    assert hist.dtype == np.uint32 and hist.shape == (5, layout["dims"]) and shape.shape == (5, lmax, 2)
    assert not _channel(hist, layout, "mbhx").any() and not _channel(hist, layout, "mbhy").any()
    hof = _channel(hist, layout, "hof")
    assert not hof[..., :8].any()
    steps_of = np.bincount([j * nt // lmax for j in range(lmax)], minlength=nt)  # the steps j of every temporal cell: 2, 1, 1
    assert steps_of.tolist() == [2, 1, 1]
    cs = N // nxy
    for i, (cx, cy) in enumerate(centres):
        crossed = length[i] - 1
        for t in range(nt):
            steps = sum(1 for j in range(crossed) if j * nt // lmax == t)
            for r in range(nxy):
                for c in range(nxy):
                    xs = np.arange(cx - N // 2 + c * cs, cx - N // 2 + (c + 1) * cs)
                    ys = np.arange(cy - N // 2 + r * cs, cy - N // 2 + (r + 1) * cs)
                    inside = int(((xs >= 0) & (xs < w)).sum() * ((ys >= 0) & (ys < h)).sum())
                    assert hof[i, t, r, c, 8] == 256 * inside * steps, (i, t, r, c)
    assert not hist[3].any()  # a track of length 1
    assert not shape.any()    # nobody moved: S == 0
    assert stats["windows"] == 4 + 4 + 2 + 0 + 1 and stats["cut"] == 4 + 2 + 0 + 1 and stats["clamped"] == 0
    # min_flow = 0: the zero vector has no octant, bin 8 stays empty
    hist0, _ = tracking.track_descriptors_ref(frames, np.zeros((npairs, h, w, 2), _f32), tracks, start, length, N, nxy, nt, 0.0)
    assert not _channel(hist0, layout, "hof").any()
    assert np.array_equal(_channel(hist0, layout, "hog"), _channel(hist, layout, "hog")) and _channel(hist, layout, "hog").any()


def test_a_constant_frame_has_no_hog():
    w, h, npairs = 12, 10, 2
    frames = np.full((npairs + 1, h, w, 3), 200, np.uint8)
    rng = np.random.default_rng(2)
    flow = rng.standard_normal((npairs, h, w, 2)).astype(_f32)
    tracks, start, length = _still_tracks([(6, 5), (0, 0)], [0, 0], [3, 3], 2)
    hist, _ = tracking.track_descriptors_ref(frames, flow, tracks, start, length, 6, 3, 2, 0.4)
    layout = tracking.descriptor_layout(6, 3, 2)
    assert not _channel(hist, layout, "hog").any()
    assert all(_channel(hist, layout, name).any() for name in ("hof", "mbhx", "mbhy"))


# ------------------------------------------------------------------ translation
def test_mbh_ignores_a_constant_added_to_an_integer_flow():
    w, h, npairs, lmax = 24, 18, 3, 3
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (npairs + 1, h, w), dtype=np.uint8)
    flow = rng.integers(-6, 7, (npairs, h, w, 2)).astype(_f32)
    tracks, start, length, _ = tracking.dense_tracks_ref(frames, np.zeros_like(flow), None, 4, 1, 0, lmax)
    layout = tracking.descriptor_layout(8, 2, 3)
    a, _ = tracking.track_descriptors_ref(frames, flow, tracks, start, length, 8, 2, 3, 0.4)
    b, _ = tracking.track_descriptors_ref(frames, flow + np.array([7, -3], _f32), tracks, start, length, 8, 2, 3, 0.4)
    for name in ("mbhx", "mbhy", "hog"):
        assert np.array_equal(_channel(a, layout, name), _channel(b, layout, name)) and _channel(a, layout, name).any()
    assert not np.array_equal(_channel(a, layout, "hof"), _channel(b, layout, "hof"))


# ------------------------------------------------------------------ by hand
def test_a_4x4_case_by_hand():
    """one track, one step, a 4x4 image and a 4x4 window with its centre at (2, 2): x = a, y = b, every pixel inside.

    frame: g[y][x] = 10 x, so gx = 20 inside and 10 in the first and last column (clamped), gy = 0: oct(20, 0) = oct(10, 0) =
    bin 0 (Q 0, q = 0 < p).  m = 20 or 10, q = 16 m = 320 or 160.  Cells of 2 x 2: each holds one border and one inner column on
    two rows: bin 0 = 2 * (160 + 320) = 960.

    flow: u = 3 y, v = -4 everywhere except v[0][0] = 0.  HOF: m = sqrt(9 y^2 + 16) = 4, 5, sqrt(52), sqrt(97) for y = 0..3; oct(u, -4):
    y = 0: a = 0 >= 0, b < 0: Q 3, (p, q) = (4, 0): bin 6; y = 1: (p, q) = (4, 3): bin 6; y = 2: (4, 6): bin 7; y = 3: (4, 9): bin 7.
    The pixel (0, 0) has (u, v) = (0, 0): m = 0 < min_flow: bin 8, q = 256.
    MBHx: gx = 0, gy = 6 inside, 3 on the first and last row: oct(0, 6): Q 1, (p, q) = (6, 0): bin 2; q = 4096 * 6 = 24576 and 12288.
    MBHy: only around (0, 0): at (1, 0): gx = v[0][2] - v[0][0] = -4, gy = 0: Q 2, (p, q) = (4, 0): bin 4, q = 16384;
    at (0, 1): gx = 0, gy = v[2][0] - v[0][0] = -4: Q 3, (p, q) = (4, 0): bin 6, q = 16384; at (0, 0): gx = v[0][1] - v[0][0] = -4,
    gy = v[1][0] - v[0][0] = -4: Q 2, (p, q) = (4, 4): bin 5, m = sqrt(32), q = floor(4096 sqrt(32) + 0.5) = 23170."""
    frames = np.tile((10 * np.arange(4)).astype(np.uint8), (2, 4, 1))
    flow = np.zeros((1, 4, 4, 2), _f32)
    flow[0, :, :, 0] = 3 * np.arange(4)[:, None]
    flow[0, :, :, 1] = -4
    flow[0, 0, 0, 1] = 0
    tracks = np.array([[[2.4, 1.5]], [[2.4, 4.5]]], _f32)  # floorf(2.4 + 0.5) = 2, floorf(1.5 + 0.5) = 2
    hist, shape = tracking.track_descriptors_ref(frames, flow, tracks, [0], [2], 4, 2, 1, 0.4)
    layout = tracking.descriptor_layout(4, 2, 1)
    want = {name: np.zeros((2, 2, bins), np.int64) for name, bins, _ in tracking.DESC_CHANNELS}
    want["hog"][:, :, 0] = 960
    q = lambda m, s: int(np.floor(np.minimum(_f32(m) * _f32(s), _f32(65535)) + _f32(0.5)))
    m = [np.sqrt(_f32(9 * y * y + 16)) for y in range(4)]
    want["hof"][0, :, 6] = 2 * q(m[0], 256) + 2 * q(m[1], 256)
    want["hof"][1, :, 7] = 2 * q(m[2], 256) + 2 * q(m[3], 256)
    want["hof"][0, 0, 6] -= q(m[0], 256)
    want["hof"][0, 0, 8] = 256
    assert q(m[0], 256) == 1024 and q(m[1], 256) == 1280
    want["mbhx"][:, :, 2] = 2 * 12288 + 2 * 24576
    want["mbhy"][0, 0, 4], want["mbhy"][0, 0, 6], want["mbhy"][0, 0, 5] = 16384, 16384, 23170
    for name in want:
        assert np.array_equal(_channel(hist, layout, name)[0, 0], want[name]), (name, _channel(hist, layout, name)[0, 0])
    assert np.array_equal(shape, np.array([[[0.0, 1.0]]], _f32))


def test_the_shape_is_the_displacements_over_their_summed_length():
    tracks = np.full((4, 3, 2), tracking.ENDED_BITS, np.uint32).view(_f32)
    tracks[:, 0] = [(5, 5), (8, 9), (8, 9), (2, 9)]   # steps (3, 4), (0, 0), (-6, 0): S = 11
    tracks[:3, 1] = [(1, 1), (1.5, 1), (1.5, 3)]      # steps (0.5, 0), (0, 2): S = 2.5; length 3
    tracks[:1, 2] = [(4, 4)]                          # length 1
    frames, flow = np.zeros((4, 12, 12), np.uint8), np.zeros((3, 12, 12, 2), _f32)
    _, shape = tracking.track_descriptors_ref(frames, flow, tracks, [0, 0, 2], [4, 3, 1], 2, 1, 1, 0.0)
    want = np.zeros((3, 3, 2), _f32)
    want[0] = np.array([(3, 4), (0, 0), (-6, 0)], _f32) / _f32(11)
    want[1, :2] = np.array([(0.5, 0), (0, 2)], _f32) / _f32(2.5)
    assert np.array_equal(shape.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------ clamped and skipped values
def test_large_and_non_finite_flows_are_clamped_and_skipped():
    w, h = 10, 8
    frames = np.zeros((2, h, w), np.uint8)
    flow = np.ones((1, h, w, 2), _f32)
    flow[0, 2, 3] = (300, 0)        # 256 * 300 > 65535: clamped in HOF, and its neighbours' MBHx
    flow[0, 5, 6] = (np.nan, 1)     # no HOF, no MBHx around it
    flow[0, 6, 2] = (1e30, 1)       # u * u overflows: not finite
    tracks, start, length = _still_tracks([(5, 4)], [0], [2], 1)
    stats = {}
    hist, _ = tracking.track_descriptors_ref(frames, flow, tracks, start, length, 16, 1, 1, 0.0, stats=stats)
    assert stats["clamped"] >= 5 and stats["skipped"] > w * h  # (HOG contributes nothing anywhere)
    layout = tracking.descriptor_layout(16, 1, 1)
    hof = _channel(hist, layout, "hof")[0, 0, 0, 0]
    assert hof[0] == 65535 and hof[1] == (w * h - 3) * 362 and hof[8] == 0  # quant(sqrt(2), 256) = 362
    assert int(hist.max()) <= 65535 * w * h


# ------------------------------------------------------------------ rotation by 90 degrees
def test_rotating_the_input_moves_every_bin_by_two():
    """The frame and the flow field turned by 90 degrees (x' = h-1-y, y' = x, vectors (u', v') = (-v, u)), the track centres with
    them.  oct(-b, a) = oct(a, b) + 2 mod 8 holds exactly, ties included: the four cases of oct map onto each other.  An even
    window is not symmetric about its centre (x = cx - N/2 .. cx + N/2 - 1), so the turned centre is (h - y, x): the window's
    pixels then map onto each other one to one.  Clamped neighbours map onto clamped neighbours.  Window cell (row r, column c)
    becomes (row c, column nxy-1-r).  No test of equality between octants is involved, so no tie can break it."""
    w, h, npairs, N, nxy, nt = 17, 13, 2, 6, 3, 2
    rng = np.random.default_rng(4)
    frames = rng.integers(0, 256, (npairs + 1, h, w, 3), dtype=np.uint8)
    flow = rng.integers(-3, 4, (npairs, h, w, 2)).astype(_f32) * _f32(0.25)   # many zeros and ties on the octant boundaries
    centres = [(8, 6), (1, 1), (16, 12), (0, 7), (9, 1), (3, 11)]
    tracks, start, length = _still_tracks(centres, [0] * 6, [3] * 6, 2)
    hist, _ = tracking.track_descriptors_ref(frames, flow, tracks, start, length, N, nxy, nt, 0.3)
    rot = lambda a: np.ascontiguousarray(np.rot90(a, k=-1, axes=(1, 2)))  # out[y'][x'] = in[h-1-x'][y'], i.e. x' = h-1-y, y' = x
    rframes, rflow = rot(frames), rot(flow)
    rflow = np.stack([-rflow[..., 1], rflow[..., 0]], -1)
    rtracks, _, _ = _still_tracks([(h - y, x) for x, y in centres], start, length, 2)
    rhist, _ = tracking.track_descriptors_ref(rframes, rflow, rtracks, start, length, N, nxy, nt, 0.3)
    layout = tracking.descriptor_layout(N, nxy, nt)
    for name in ("hog", "hof", "mbhx", "mbhy"):
        # the turned field's u' = -v, v' = u: MBHx of the turned input is MBHy of the original (the sign does not move m, and
        # oct(-a, -b) = oct(a, b) + 4), MBHy of the turned input is MBHx of the original
        src = {"hog": "hog", "hof": "hof", "mbhx": "mbhy", "mbhy": "mbhx"}[name]
        a, b = _channel(hist, layout, src), _channel(rhist, layout, name)
        assert a.any()
        moved = np.zeros_like(a)
        for r in range(nxy):
            for c in range(nxy):
                moved[:, :, c, nxy - 1 - r, :8] = np.roll(a[:, :, r, c, :8], 6 if name == "mbhx" else 2, axis=-1)
                if name == "hof":
                    moved[:, :, c, nxy - 1 - r, 8] = a[:, :, r, c, 8]
        assert np.array_equal(b, moved), name


# ------------------------------------------------------------------ normalisation
def test_normalize_descriptors():
    layout = tracking.descriptor_layout(4, 2, 1)
    rng = np.random.default_rng(5)
    hist = rng.integers(0, 70000, (3, layout["dims"])).astype(np.uint32)
    off, bins = layout["channels"]["mbhx"]
    hist[1, off:off + bins * 4] = 0      # an empty channel
    hist[2] = 0                          # an empty descriptor
    l2 = tracking.normalize_descriptors(hist, layout, "l2")
    rs = tracking.normalize_descriptors(hist, layout, "rootsift")
    assert l2.dtype == rs.dtype == np.float64 and l2.shape == rs.shape == hist.shape
    for name, (off, bins) in layout["channels"].items():
        sl = slice(off, off + bins * 4)
        for i in range(3):
            v = hist[i, sl].astype(np.float64)
            if v.any():
                assert np.allclose(l2[i, sl], v / np.linalg.norm(v), rtol=1e-14, atol=0)
                assert np.allclose(rs[i, sl], np.sqrt(v / v.sum()), rtol=1e-14, atol=0)
                assert abs(np.linalg.norm(l2[i, sl]) - 1) < 1e-12 and abs(np.linalg.norm(rs[i, sl]) - 1) < 1e-12
            else:
                assert not l2[i, sl].any() and not rs[i, sl].any()
    with pytest.raises(ValueError):
        tracking.normalize_descriptors(hist, layout, "l1")
