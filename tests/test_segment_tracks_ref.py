"""CPU: of_dis_amd/segments.py: segment_overlap_ref, segment_link_ref, segment_chain_ref, segment_relabel_ref and
segment_tracks_ref, the numpy statement of include/ofdis.h's section "Object tracks", on cases small enough that every outcome
is written out by hand here.  The device calls against this model: tests/test_gpu_segment_tracks.py."""
import numpy as np
import pytest

from of_dis_amd import segments as S

_f32 = np.float32


def _info(*counts):
    """info of label_segments with info[:, 2] = counts"""
    info = np.zeros((len(counts), 4), np.int64)
    info[:, 2] = counts
    return info


def _records(areas, S_):
    """records [N, S, 12] with the given areas per map and distinct values in the summed fields: field f of (k, s) is
    1000 * f + 10 * k + s for f = 6 .. 10"""
    rec = np.zeros((len(areas), S_, 12), np.int64)
    for k, row in enumerate(areas):
        for s, a in enumerate(row, 1):
            rec[k, s - 1, 0] = a
            for f in range(6, 11):
                rec[k, s - 1, f] = 1000 * f + 10 * k + s
    return rec


def _pair(c, S_=3):
    """overlap [1, S, S] of one pair from a small matrix"""
    ov = np.zeros((1, S_, S_), np.int32)
    c = np.asarray(c, np.int32)
    ov[0, :c.shape[0], :c.shape[1]] = c
    return ov


# ------------------------------------------------------------------ overlap
def test_overlap_by_hand():
    """4x2, every pixel moves one to the right except two of segment 2: -1.5 rounds to -2 and -0.5 to -0 (to even)"""
    seg = np.array([[[1, 1, 0, 2], [1, 0, 0, 2]], [[0, 1, 1, 2], [0, 1, 0, 2]]], np.int32)
    flow = np.zeros((2, 2, 4, 2), _f32)
    flow[0, ..., 0] = 1.0
    flow[0, 0, 3, 0], flow[0, 1, 3, 0] = -1.5, -0.5
    flow[1] = np.nan   # the flow of the last map is never read
    ov = S.segment_overlap_ref(seg, flow, _info(2, 2), 2)
    assert ov.tolist() == [[[3, 0], [1, 1]]]
    flow[0, 0, 3, 0] = 1.0   # leaves the frame
    assert S.segment_overlap_ref(seg, flow, _info(2, 2), 2).tolist() == [[[3, 0], [0, 1]]]
    flow[0, 0, 0] = (np.nan, 0.0)   # unusable
    flow[0, 0, 1] = (0.0, np.nextafter(_f32(4096.0), _f32(np.inf)))
    assert S.segment_overlap_ref(seg, flow, _info(2, 2), 2).tolist() == [[[1, 0], [0, 1]]]


def test_overlap_counts_only_recorded_values_and_keeps_the_fill():
    seg = np.array([[[1, 2, 3, -1]], [[1, 2, 3, 7]]], np.int32)
    flow = np.zeros((2, 1, 4, 2), _f32)
    fill = np.full((1, 3, 3), -9, np.int32)
    ov = S.segment_overlap_ref(seg, flow, _info(2, 5), 3, overlap_fill=fill)   # n_0 = 2, n_1 = min(5, 3) = 3
    assert ov.tolist() == [[[1, 0, 0], [0, 1, 0], [-9, -9, -9]]]
    ov = S.segment_overlap_ref(seg, flow, _info(3, -4), 3, overlap_fill=fill)  # n_1 = 0: nothing is defined
    assert (ov == -9).all()


# ------------------------------------------------------------------ link
def test_link_a_tie_goes_to_the_smallest_index():
    rec = _records([[10, 10, 10], [10, 10, 10]], 3)
    assert S.segment_link_ref(_pair([[5, 5, 0]]), rec, _info(3, 3), 3, 0).tolist() == [[1, 0, 0]]
    assert S.segment_link_ref(_pair([[0, 0], [4, 0], [4, 0]]), rec, _info(3, 3), 3, 0).tolist() == [[0, 1, 0]]


def test_link_rejects_a_best_that_is_not_mutual():
    rec = _records([[10, 10, 10], [10, 10, 10]], 3)
    # fbest(1) = 1 but bbest(1) = 2; fbest(2) = 1 and bbest(1) = 2
    assert S.segment_link_ref(_pair([[5, 0, 0], [6, 1, 0]]), rec, _info(3, 3), 3, 0).tolist() == [[0, 1, 0]]


def test_link_min_share_at_the_exact_boundary():
    rec = _records([[50], [60]], 3)   # the smaller area is 50: 90 % of it is 45
    assert S.segment_link_ref(_pair([[45]]), rec, _info(1, 1), 3, 90).tolist() == [[1, 0, 0]]
    assert S.segment_link_ref(_pair([[44]]), rec, _info(1, 1), 3, 90).tolist() == [[0, 0, 0]]
    assert S.segment_link_ref(_pair([[44]]), rec, _info(1, 1), 3, 88).tolist() == [[1, 0, 0]]
    assert S.segment_link_ref(_pair([[1]]), rec, _info(1, 1), 3, 0).tolist() == [[1, 0, 0]]
    assert S.segment_link_ref(_pair([[0]]), rec, _info(1, 1), 3, 0).tolist() == [[0, 0, 0]]   # c > 0 is asked for even at 0 %
    rec[0, 0, 0], rec[1, 0, 0] = -5, 1 << 40   # areas clamp to 0 .. 2^26
    assert S.segment_link_ref(_pair([[1]]), rec, _info(1, 1), 3, 100).tolist() == [[1, 0, 0]]


def test_link_keeps_the_fill_beyond_n():
    rec = _records([[10, 10, 10], [10, 10, 10]], 3)
    link = S.segment_link_ref(_pair([[5, 0], [0, 3]]), rec, _info(2, 2), 3, 0, link_fill=np.full((1, 3), 77, np.int32))
    assert link.tolist() == [[1, 2, 77]]


def test_links_are_injective():
    rng = np.random.default_rng(5)
    for trial in range(20):
        n0, n1 = rng.integers(1, 9, 2)
        ov = np.zeros((1, 8, 8), np.int32)
        ov[0] = rng.integers(0, 4, (8, 8)) * rng.integers(0, 2, (8, 8))   # many ties, many zeros
        rec = np.zeros((2, 8, 12), np.int64)
        rec[:, :, 0] = rng.integers(1, 6, (2, 8))
        link = S.segment_link_ref(ov, rec, _info(n0, n1), 8, int(rng.integers(0, 101)))[0, :n0]
        hit = link[link > 0]
        assert len(set(hit.tolist())) == len(hit) and (hit <= n1).all(), (trial, link)


# ------------------------------------------------------------------ chain
def test_chain_split_merge_and_birth_after_map_0():
    """three maps.  Pair 0: segment 1 splits into 1 (30 pixels) and 2 (20): the larger piece goes on, the smaller is born.
    Pair 1: segments 1 and 2 merge into 1: the larger overlap goes on, the other track ends; segment 2 of map 2 is new."""
    rec = _records([[50], [30, 20], [50, 9]], 3)
    info = _info(1, 2, 2)
    ov = np.concatenate([_pair([[30, 20]]), _pair([[30, 0], [20, 0]])])
    link = S.segment_link_ref(ov, rec, info, 3, 0)
    assert link.tolist() == [[1, 0, 0], [1, 0, 0]]
    fill = np.full((3, 3), -1, np.int32)
    ids, tracks, tinfo = S.segment_chain_ref(link, rec, info, 3, 8, ids_fill=fill, tracks_fill=np.full((8, 12), -2, np.int64))
    # numbered by (k, s): (0, 1) -> 1, (1, 2) -> 2, (2, 2) -> 3
    assert ids.tolist() == [[1, -1, -1], [1, 2, -1], [1, 3, -1]]
    assert tinfo.tolist() == [3, 3, 2, 3]
    f = lambda k, s: [1000 * i + 10 * k + s for i in range(6, 11)]
    sums = [sum(x) for x in zip(f(0, 1), f(1, 1), f(2, 1))]
    assert tracks[0].tolist() == [0, 1, 3, 1, 130] + sums + [30, 50]
    assert tracks[1].tolist() == [1, 2, 1, 2, 20] + f(1, 2) + [20, 20]
    assert tracks[2].tolist() == [2, 2, 1, 2, 9] + f(2, 2) + [9, 9]
    assert (tracks[3:] == -2).all()


def test_chain_numbers_by_map_then_segment_and_truncates_the_records():
    rec = _records([[5, 6, 7], [5, 6, 7]], 3)
    info = _info(3, 3)
    link = np.array([[0, 3, 0]], np.int32)   # (0, 2) -> (1, 3); (1, 1) and (1, 2) are born
    ids, tracks, tinfo = S.segment_chain_ref(link, rec, info, 3, 4, tracks_fill=np.full((4, 12), -2, np.int64))
    assert ids.tolist() == [[1, 2, 3], [4, 5, 2]]
    assert tinfo.tolist() == [5, 4, 1, 2]
    assert tracks[:, :4].tolist() == [[0, 1, 1, 1], [0, 2, 2, 3], [0, 3, 1, 3], [1, 1, 1, 1]]
    assert tracks[1, 4] == 6 + 7 and tracks[1, 10:].tolist() == [6, 7]


def test_chain_ignores_links_out_of_range_and_takes_the_smallest_predecessor():
    rec = _records([[5, 6, 7], [5, 6]], 3)
    info = _info(3, 2)
    link = np.array([[3, 2, 2]], np.int32)   # 3 > n_1; two a claim b = 2 (no link step gives that): the smaller a is it
    ids, tracks, tinfo = S.segment_chain_ref(link, rec, info, 3, 8)
    assert ids.tolist() == [[1, 2, 3], [4, 2, 0]]
    assert tinfo.tolist() == [4, 4, 1, 2]


def test_chain_sums_wrap():
    rec = _records([[1], [1]], 1)
    rec[:, 0, 9] = (1 << 62) + 5   # squ: twice this passes 2^63
    ids, tracks, tinfo = S.segment_chain_ref(np.array([[1]], np.int32), rec, _info(1, 1), 1, 1)
    assert tracks[0, 8] == -(1 << 63) + 10 and tinfo.tolist() == [1, 1, 1, 2]


def test_one_map():
    seg = np.array([[[1, 2, 0, 5]]], np.int32)
    rec = _records([[5, 6]], 4)
    ids, tracks, tinfo, tmap = S.segment_tracks_ref(seg, np.zeros((1, 1, 4, 2), _f32), rec, _info(2), 4, 50, 8)
    assert ids.tolist() == [[1, 2, 0, 0]] and tinfo.tolist() == [2, 2, 0, 1]
    assert tracks[:2, :5].tolist() == [[0, 1, 1, 1, 5], [0, 2, 1, 2, 6]]
    assert tmap.tolist() == [[[1, 2, 0, 0]]]   # 5 > n_0: background


# ------------------------------------------------------------------ relabel, the whole
def test_relabel():
    seg = np.array([[[0, 1, 2, 3, -1]], [[2, 2, 1, 9, 0]]], np.int32)
    ids = np.array([[4, 5, 6], [7, 8, 9]], np.int32)
    assert S.segment_relabel_ref(seg, ids, _info(2, 3), 3).tolist() == [[[0, 4, 5, 0, 0]], [[8, 8, 7, 0, 0]]]


def test_the_whole_on_a_moving_block():
    """a 2x2 block moving one pixel right per map over three maps, and a block that appears in map 1"""
    seg = np.zeros((3, 4, 8), np.int32)
    for k in range(3):
        seg[k, 0:2, k:k + 2] = 1
    seg[1, 3, 5:8] = 2
    seg[2, 3, 5:8] = 2
    flow = np.zeros((3, 4, 8, 2), _f32)
    flow[:, 0:2, :, 0] = 1.0
    rec = _records([[4], [4, 3], [4, 3]], 2)
    ids, tracks, tinfo, tmap = S.segment_tracks_ref(seg, flow, rec, _info(1, 2, 2), 2, 100, 4)
    assert ids.tolist() == [[1, 0], [1, 2], [1, 2]] and tinfo.tolist() == [2, 2, 3, 3]
    assert tracks[:2, :5].tolist() == [[0, 1, 3, 1, 12], [1, 2, 2, 2, 6]]
    assert (tmap == np.where(seg == 1, 1, np.where(seg == 2, 2, 0))).all()


def test_rejected_arguments_and_work_bytes():
    seg, flow = np.zeros((1, 1, 1), np.int32), np.zeros((1, 1, 1, 2), _f32)
    for bad in (dict(max_segments=0), dict(max_segments=1025)):
        with pytest.raises(ValueError):
            S.segment_overlap_ref(seg, flow, _info(0), **bad)
    with pytest.raises(ValueError):
        S.segment_link_ref(np.zeros((0, 1, 1), np.int32), _records([[1]], 1), _info(1), 1, 101)
    with pytest.raises(ValueError):
        S.segment_chain_ref(np.zeros((0, 1), np.int32), _records([[1]], 1), _info(1), 1, 0)
    assert S.segment_tracks_work_bytes(1, 1) == 8 and S.segment_tracks_work_bytes(2, 1) == 8
    assert S.segment_tracks_work_bytes(2, 2) == 24 and S.segment_tracks_work_bytes(3, 3) == 96
    assert S.segment_tracks_work_bytes(4, 5) == 360 and S.segment_tracks_work_bytes(65536, 1024) == 65535 * 1024 * 1025 * 4
    for bad in ((0, 4), (65537, 4), (2, 0), (2, 1025)):
        assert S.segment_tracks_work_bytes(*bad) == 0
