"""CPU: properties of the numpy statement of the motion-compensated temporal filter (of_dis_amd/temporal.py:
temporal_filter_ref, the definition of include/ofdis.h: ofdis_temporal_filter, operation by operation in float32).  The kernels
are compared with it bit for bit in tests/test_gpu_tfilter.py; here the statement itself is held to what the header promises."""
import numpy as np
import pytest

from of_dis_amd import temporal
from of_dis_amd.temporal import SUPPORT_NEXT, SUPPORT_PREV, temporal_filter_ref
from seq_products import FLT_MIN

_f32 = np.float32


def _frames(rng, n, h, w, noc):
    return rng.integers(0, 256, (n, h, w) + ((3,) if noc == 3 else ()), dtype=np.uint8)


def _zero_flows(npairs, h, w):
    z = np.zeros((npairs, h, w, 2), _f32)
    return z, z.copy()


@pytest.mark.parametrize("noc", [1, 3])
def test_wn_zero_returns_the_clip(noc):
    """whatever the flows, the masks and tau"""
    rng = np.random.default_rng(1 + noc)
    frames = _frames(rng, 4, 9, 13, noc)
    fw = (rng.standard_normal((3, 9, 13, 2)) * 2).astype(_f32)
    rev = (rng.standard_normal((3, 9, 13, 2)) * 2).astype(_f32)
    fw[0, 0, 0], rev[1, 2, 3] = np.nan, np.inf
    masks = rng.integers(0, 3, (2, 3, 9, 13), dtype=np.uint8)
    for tau in (np.inf, 8.0, FLT_MIN):
        for m in ((None, None), tuple(masks)):
            out, support = temporal_filter_ref(frames, fw, rev, *m, wn=0.0, tau=tau)
            assert out.dtype == np.uint8 and out.shape == frames.shape and np.array_equal(out, frames)
            assert support.shape == (4, 9, 13) and not support.any()


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("tau", [np.inf, 8.0])
def test_identical_frames_with_zero_flows_return_the_clip(noc, tau):
    rng = np.random.default_rng(3 + noc)
    frames = np.repeat(_frames(rng, 1, 11, 17, noc), 4, axis=0)
    out, support = temporal_filter_ref(frames, *_zero_flows(3, 11, 17), wn=1.0, tau=tau)
    assert np.array_equal(out, frames)
    assert (support[0] == SUPPORT_NEXT).all() and (support[3] == SUPPORT_PREV).all()
    assert (support[1:3] == (SUPPORT_PREV | SUPPORT_NEXT)).all()


def _shifted_clip(rng, n, h, w, noc, d):
    """frame k = one large image cut out at -k * d: frame k+1 at x + d shows what frame k shows at x"""
    dx, dy = d
    mx, my = abs(dx) * n, abs(dy) * n
    big = _frames(rng, 1, h + 2 * my, w + 2 * mx, noc)[0]
    return np.stack([big[my - k * dy:my - k * dy + h, mx - k * dx:mx - k * dx + w] for k in range(n)])


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("d", [(3, -2), (-4, 1), (2, 0), (0, 5)])
def test_integer_translation(noc, d):
    """Ffw = d, Frev = -d on exact shifts of one image: each frame comes back unchanged wherever both samples are inside, and
    at the pixels whose sample falls outside `support` drops exactly that candidate's bit"""
    n, h, w = 4, 14, 19
    dx, dy = d
    rng = np.random.default_rng(7 + noc)
    frames = _shifted_clip(rng, n, h, w, noc, d)
    fw = np.broadcast_to(np.array(d, _f32), (n - 1, h, w, 2)).copy()
    ys, xs = np.mgrid[0:h, 0:w]
    next_in = (xs + dx >= 0) & (xs + dx <= w - 1) & (ys + dy >= 0) & (ys + dy <= h - 1)
    prev_in = (xs - dx >= 0) & (xs - dx <= w - 1) & (ys - dy >= 0) & (ys - dy <= h - 1)
    assert (next_in & prev_in).any() and not next_in.all() and not prev_in.all()
    for tau in (np.inf, 8.0):
        out, support = temporal_filter_ref(frames, fw, -fw, wn=1.0, tau=tau)
        for f in range(n):
            want = (SUPPORT_NEXT * next_in if f < n - 1 else 0) | (SUPPORT_PREV * prev_in if f > 0 else 0)
            assert np.array_equal(support[f], want), (d, f)
            both = next_in & prev_in
            assert np.array_equal(out[f][both], frames[f][both]), (d, f)
        # exact shifts: a pixel averaged with copies of itself is itself, with one neighbour or two
        assert np.array_equal(out, frames)


def test_a_mask_code_removes_exactly_that_candidate():
    n, h, w = 3, 8, 10
    rng = np.random.default_rng(11)
    frames = np.repeat(_frames(rng, 1, h, w, 1), n, axis=0)
    fw, rev = _zero_flows(n - 1, h, w)
    mfw, mrev = np.zeros((n - 1, h, w), np.uint8), np.zeros((n - 1, h, w), np.uint8)
    mfw[1, 2, 3], mfw[0, 4, 5] = 1, 2      # frame 1 -> 2 at (3, 2); frame 0 -> 1 at (5, 4)
    mrev[0, 2, 3], mrev[1, 6, 7] = 2, 1    # frame 1 -> 0 at (3, 2); frame 2 -> 1 at (7, 6)
    full = np.full((n, h, w), SUPPORT_PREV | SUPPORT_NEXT, np.uint8)
    full[0], full[n - 1] = SUPPORT_NEXT, SUPPORT_PREV
    _, support = temporal_filter_ref(frames, fw, rev, mfw, mrev)
    want = full.copy()
    want[1, 2, 3] = 0
    want[0, 4, 5] = 0
    want[2, 6, 7] = 0
    assert np.array_equal(support, want)
    _, support = temporal_filter_ref(frames, fw, rev, mfw, None)
    want = full.copy()
    want[1, 2, 3] = SUPPORT_PREV
    want[0, 4, 5] = 0
    assert np.array_equal(support, want)
    _, support = temporal_filter_ref(frames, fw, rev, None, mrev)
    want = full.copy()
    want[1, 2, 3] = SUPPORT_NEXT
    want[2, 6, 7] = 0
    assert np.array_equal(support, want)


def test_a_masked_candidate_does_not_enter_the_average():
    frames = np.array([[[10]], [[100]], [[250]]], np.uint8)
    fw, rev = _zero_flows(2, 1, 1)
    out, support = temporal_filter_ref(frames, fw, rev)
    assert out[:, 0, 0].tolist() == [55, 120, 175] and support[:, 0, 0].tolist() == [2, 3, 1]
    mfw = np.array([[[0]], [[1]]], np.uint8)
    out, support = temporal_filter_ref(frames, fw, rev, mfw, None)
    assert out[:, 0, 0].tolist() == [55, 55, 175] and support[:, 0, 0].tolist() == [2, 1, 1]


@pytest.mark.parametrize("noc", [1, 3])
def test_tau_gates_a_neighbour_that_differs_by_at_least_tau(noc):
    """the largest channel difference d decides: d >= tau gives weight 0 and `support` loses the bit, d < tau keeps it"""
    h, w, tau = 4, 6, 8.0
    base = np.full((h, w) + ((3,) if noc == 3 else ()), 100, np.uint8)
    nxt, prv = base.copy(), base.copy()
    ch = (..., 2) if noc == 3 else (...,)
    nxt[(0, 0) + ch[1:]] = 108      # d = tau
    nxt[(0, 1) + ch[1:]] = 107      # d < tau
    nxt[(0, 2) + ch[1:]] = 91       # d > tau, downwards
    prv[(1, 0) + ch[1:]] = 92       # d = tau
    prv[(1, 1) + ch[1:]] = 93
    frames = np.stack([prv, base, nxt])
    out, support = temporal_filter_ref(frames, *_zero_flows(2, h, w), wn=1.0, tau=tau)
    want = np.full((h, w), SUPPORT_PREV | SUPPORT_NEXT, np.uint8)
    want[0, 0] = want[0, 2] = SUPPORT_PREV
    want[1, 0] = SUPPORT_NEXT
    assert np.array_equal(support[1], want)
    assert np.array_equal(out[1][support[1] != 3], base[support[1] != 3])   # the other neighbour equals the frame
    # tau = FLT_MIN: only a neighbour that equals the pixel in every channel survives
    _, support = temporal_filter_ref(frames, *_zero_flows(2, h, w), wn=1.0, tau=FLT_MIN)
    want = np.full((h, w), SUPPORT_PREV | SUPPORT_NEXT, np.uint8)
    want[0, 0:3] = SUPPORT_PREV
    want[1, 0:2] = SUPPORT_NEXT
    assert np.array_equal(support[1], want)
    # tau = +inf: no gate at all
    _, support = temporal_filter_ref(frames, *_zero_flows(2, h, w), wn=1.0, tau=np.inf)
    assert (support[1] == 3).all()


def test_the_gate_fades_the_weight_linearly():
    """c = 100, next = 104, tau = 8, wn = 1: g = 0.5, out = floor((100 + 0.5 * 104) / 1.5 + 0.5) = 101"""
    frames = np.array([[[100]], [[104]]], np.uint8)
    out, support = temporal_filter_ref(frames, *_zero_flows(1, 1, 1), wn=1.0, tau=8.0)
    assert out[:, 0, 0].tolist() == [101, 103] and support[:, 0, 0].tolist() == [2, 1]
    out, _ = temporal_filter_ref(frames, *_zero_flows(1, 1, 1), wn=0.5, tau=np.inf)
    assert out[:, 0, 0].tolist() == [101, 103]     # (100 + 52) / 1.5 = 101.33, (104 + 50) / 1.5 = 102.67


@pytest.mark.parametrize("noc", [1, 3])
def test_the_end_frames_have_one_neighbour(noc):
    rng = np.random.default_rng(17 + noc)
    n, h, w = 5, 7, 9
    frames = _frames(rng, n, h, w, noc)
    fw = (rng.standard_normal((n - 1, h, w, 2)) * 1.5).astype(_f32)
    rev = (rng.standard_normal((n - 1, h, w, 2)) * 1.5).astype(_f32)
    out, support = temporal_filter_ref(frames, fw, rev)
    assert (support[0] & SUPPORT_PREV == 0).all() and (support[n - 1] & SUPPORT_NEXT == 0).all()
    assert (support[0] & SUPPORT_NEXT).any() and (support[n - 1] & SUPPORT_PREV).any()
    assert (support[1:n - 1] == 3).any()
    # a single pair: both frames are end frames
    out, support = temporal_filter_ref(frames[:2], fw[:1], rev[:1])
    assert (support[0] & SUPPORT_PREV == 0).all() and (support[1] & SUPPORT_NEXT == 0).all()


def test_non_finite_flows_count_as_outside():
    frames = np.full((2, 3, 4), 50, np.uint8)
    fw, rev = _zero_flows(1, 3, 4)
    fw[0, 0, 0, 0], fw[0, 0, 1, 1], fw[0, 0, 2, 0], fw[0, 1, 0, 0] = np.nan, np.inf, -np.inf, 1e30
    out, support = temporal_filter_ref(frames, fw, rev)
    want = np.full((3, 4), SUPPORT_NEXT, np.uint8)
    want[0, 0:3] = want[1, 0] = 0
    assert np.array_equal(support[0], want) and np.array_equal(out, frames)


def test_the_sample_is_the_bilinear_expression_of_the_interpolation():
    """a quarter-pixel position: every product is exact, so the blend can be written down"""
    I = np.array([[[0], [40]], [[80], [200]]], np.uint8)
    got = temporal.sample(I, np.array([0.25], _f32), np.array([0.5], _f32))
    assert got.tolist() == [[(0 * 0.75 + 40 * 0.25) * 0.5 + (80 * 0.75 + 200 * 0.25) * 0.5]]
