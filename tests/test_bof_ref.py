"""CPU: the numpy model of the bag-of-features encoding (of_dis_amd/tracking.py: normalize_descriptors_u8, codebook_assign_ref,
bof_ref) against plain Python integers and against the float normalisation it quantises.  The kernels are held to this model
bit for bit in tests/test_gpu_bof.py."""
import math

import numpy as np
import pytest

from of_dis_amd import tracking

S2 = tracking.BOF_SCALE ** 2
# (patch, nxy, nt): channels of 8/9, 96/108 and 1024/1152 entries; of 24/27 in rows of 99 bytes (C = 3: odd, the channels start
# at odd offsets) and of 216/243 in rows of 891 (C = 27: odd, and in the range of the middle assignment kernel)
LAYOUTS = [(8, 1, 1), (8, 2, 3), (8, 4, 8), (8, 1, 3), (12, 3, 3)]


def _isqrt_rows(hist, layout):
    """min(255, isqrt(510^2 h // S)) in Python integers, per channel"""
    out = np.zeros(hist.shape, np.uint8)
    for seg in tracking._channel_slices(layout):
        for i, row in enumerate(hist[:, seg].tolist()):
            S = sum(row)
            if S:
                out[i, seg] = [min(255, math.isqrt(S2 * h // S)) for h in row]
    return out


def _rows(layout, rng):
    """random rows of every magnitude, and the extreme ones"""
    D = layout["dims"]
    top = 2 ** 32 - 1
    rows = [rng.integers(0, 2 ** int(b), D, dtype=np.uint64) for b in (1, 3, 8, 16, 24, 32, 32)]
    rows.append(rng.integers(0, 2 ** 32, D, dtype=np.uint64) * (rng.random(D) < 0.1))   # sparse: large shares of the sum
    rows.append(np.full(D, top, np.uint64))                                             # the largest sum there is
    rows.append(np.zeros(D, np.uint64))                                                 # all zero
    one = np.zeros(D, np.uint64)
    for seg, v in zip(tracking._channel_slices(layout), (1, top, 77, top - 1)):         # one nonzero entry per channel
        one[seg.start + (seg.stop - seg.start) // 2] = v
    rows.append(one)
    near = rng.integers(top - 5, top + 1, D, dtype=np.uint64)                           # entries near 2^32 and zeros
    near[::3] = 0
    rows.append(near)
    quarter = np.full(D, 3, np.uint64)                                                  # an entry of exactly a quarter of its sum: 255
    for seg in tracking._channel_slices(layout):
        quarter[seg.start] = seg.stop - seg.start - 1
    rows.append(quarter)
    return np.stack(rows).astype(np.uint32)


@pytest.mark.parametrize("case", LAYOUTS, ids=lambda c: f"{c[1]}x{c[1]}x{c[2]}")
def test_the_division_free_definition_is_the_integer_square_root(case):
    layout = tracking.descriptor_layout(*case)
    hist = _rows(layout, np.random.default_rng(510))
    got = tracking.normalize_descriptors_u8(hist, layout)
    assert got.dtype == np.uint8 and got.shape == hist.shape
    assert np.array_equal(got, _isqrt_rows(hist, layout))
    one, zero = got[10], got[9]
    assert (zero == 0).all()
    for seg in tracking._channel_slices(layout):
        assert one[seg].max() == one[seg].astype(int).sum() == 255                         # one nonzero entry: 255, the rest 0
        assert got[12, seg.start] == 255
    assert (got == 255).any() and ((got > 0) & (got < 255)).any()


def test_known_values():
    layout = tracking.descriptor_layout(8, 1, 1)
    hist = np.full((1, 33), 7, np.uint32)
    got = tracking.normalize_descriptors_u8(hist, layout)[0]
    assert (got[:8] == 180).all() and (got[8:17] == math.isqrt(S2 // 9)).all() and (got[17:] == 180).all()
    assert np.array_equal(got, tracking.normalize_descriptors_u8(hist * 1000, layout)[0])  # a common factor changes nothing


@pytest.mark.parametrize("case", LAYOUTS, ids=lambda c: f"{c[1]}x{c[1]}x{c[2]}")
def test_within_a_unit_of_rootsift(case):
    layout = tracking.descriptor_layout(*case)
    hist = _rows(layout, np.random.default_rng(7))
    got = tracking.normalize_descriptors_u8(hist, layout).astype(np.float64)
    want = tracking.BOF_SCALE * tracking.normalize_descriptors(hist, layout, "rootsift")
    free = want < 255  # not clamped
    assert free.sum() > free.size // 2
    # floor(sqrt(floor(t))) <= sqrt(t) < floor(sqrt(floor(t))) + 1; 1e-6 for the float64 roundings of `want`
    assert (got[free] <= want[free] + 1e-6).all() and (want[free] < got[free] + 1 + 1e-6).all()
    assert (got[~free] == 255).all()


def _brute(desc, layout, codebook):
    words, dist = [], []
    for row in desc.astype(int).tolist():
        w, d = [], []
        for seg in tracking._channel_slices(layout):
            ds = [sum((a - b) ** 2 for a, b in zip(row[seg], cw[seg])) for cw in codebook.astype(int).tolist()]
            d.append(min(ds))
            w.append(ds.index(min(ds)))
        words.append(w)
        dist.append(d)
    return np.array(words, np.int32), np.array(dist, np.int32)


def test_assignment_is_the_first_minimum():
    _first_minimum((8, 2, 1))


@pytest.mark.parametrize("case", [(8, 1, 3), (12, 3, 3)], ids=lambda c: f"{c[1]}x{c[1]}x{c[2]}")
def test_assignment_is_the_first_minimum_in_rows_of_odd_length(case):
    """the model's channel slicing where the rows are unaligned: 99 and 891 bytes"""
    _first_minimum(case)


def _first_minimum(case):
    layout = tracking.descriptor_layout(*case)
    rng = np.random.default_rng(3)
    D = layout["dims"]
    desc = rng.integers(0, 256, (9, D)).astype(np.uint8)
    codebook = rng.integers(0, 256, (6, D)).astype(np.uint8)
    codebook = np.concatenate([codebook, codebook[[2, 0]], desc[[4, 4]]])  # duplicated rows; a descriptor itself, twice
    # two rows equidistant from descriptor 0 in channel 0: one entry up by 3, another down by 3
    for k, delta in ((10, 3), (11, -3)):
        row = desc[0].astype(int)
        e = 5 if delta > 0 else 6
        row[e] = row[e] + delta if 0 <= row[e] + delta <= 255 else row[e] - delta
        codebook = np.concatenate([codebook, row[None].astype(np.uint8)])
    words, dist = tracking.codebook_assign_ref(desc, layout, codebook)
    bw, bd = _brute(desc, layout, codebook)
    assert np.array_equal(words, bw) and np.array_equal(dist, bd)
    assert words.dtype == dist.dtype == np.int32
    assert (words[4] == 8).all() and (dist[4] == 0).all()        # the first copy, never row 9
    assert words[0, 0] == 10 and dist[0, 0] == 9                 # the first of the equidistant pair
    assert not np.isin(words, (6, 7, 9)).any()                   # a later copy is never used ...
    assert not (words[:, 1:] == 11).any()                        # ... nor row 11 where it equals row 10
    # the corner of the signed domain
    lo, hi = np.zeros((1, D), np.uint8), np.full((1, D), 255, np.uint8)
    w, d = tracking.codebook_assign_ref(np.concatenate([lo, hi]), layout, np.concatenate([hi, lo]))
    assert w.tolist() == [[1] * 4, [0] * 4] and (d == 0).all()
    w, d = tracking.codebook_assign_ref(lo, layout, hi)
    C = case[1] * case[1] * case[2]
    assert d.tolist() == [[8 * C * 255 ** 2, 9 * C * 255 ** 2, 8 * C * 255 ** 2, 8 * C * 255 ** 2]]


def test_bof_columns_sum_to_the_counted_tracks():
    rng = np.random.default_rng(11)
    words = rng.integers(0, 37, (500, 4)).astype(np.int32)
    length = rng.integers(1, 5, 500).astype(np.int32)
    for min_len in (1, 3, 4, 5):
        bof = tracking.bof_ref(words, length, 37, min_len)
        assert bof.dtype == np.uint32 and bof.shape == (4, 37)
        assert (bof.sum(1) == (length >= min_len).sum()).all()
        for c in range(4):
            for k in (0, 17, 36):
                assert bof[c, k] == ((words[:, c] == k) & (length >= min_len)).sum()
    assert tracking.bof_ref(words[:0], length[:0], 5).tolist() == [[0] * 5] * 4
    odd = np.array([[0, 5, -1, 2]], np.int32)  # words outside the codebook are not counted
    assert tracking.bof_ref(odd, np.ones(1, np.int32), 5).sum(1).tolist() == [1, 0, 0, 1]
