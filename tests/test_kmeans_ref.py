"""CPU: the numpy statement of the codebook training (of_dis_amd/tracking.py: codebook_seed_ref, codebook_update_ref,
codebook_train_ref; include/ofdis.h: ofdis_codebook_seed, ofdis_codebook_update, ofdis_codebook_train) on its own: the known
values, the seeding walk, the members, empty words, the order of the slots, and the consequences the header states -- monotone
distortion, the fixed point, the route.  The descriptors are those of tests/test_gpu_bof.py (200 synthetic rows per size).  The
kernels against this model: tests/test_gpu_kmeans.py."""
import numpy as np
import pytest

from of_dis_amd import tracking
from test_gpu_bof import LMAX, _data


def _layout(nxy=1, nt=1):
    return tracking.descriptor_layout(12, nxy, nt)   # (12: a patch every nxy divides)


def _rows(values, layout=None):
    """one row per value, every entry of the row that value"""
    layout = layout or _layout()
    return np.repeat(np.asarray(values, np.uint8)[:, None], layout["dims"], 1)


# ------------------------------------------------------------------ known values
@pytest.mark.parametrize("members,mean", [([0, 1], 1), ([0, 0, 1], 0), ([254, 255], 255), ([7], 7), ([0, 255], 128),
                                          ([1, 2, 2], 2), ([1, 1, 2], 1), ([255] * 5, 255)])
def test_the_mean_is_rounded_half_up(members, mean):
    layout = _layout()
    desc = _rows(members)
    words = np.zeros((len(members), 4), np.int32)
    cb, counts = tracking.codebook_update_ref(desc, layout, words, None, _rows([99]))
    assert (cb == mean).all() and (counts == len(members)).all()


SIZES = [(1, 1), (2, 3), (1, 3), (3, 3)]   # C = 1, 12; 3 and 27: rows of odd length, 27 in the range of the middle assignment kernel


@pytest.mark.parametrize("size", SIZES)
def test_one_word_is_the_rounded_mean_of_the_members_after_one_iteration(size):
    layout, _, length, desc, _ = _data(*size)
    for ln, min_len in ((None, 1), (length, LMAX + 1)):
        member = np.ones(len(desc), bool) if ln is None else ln >= min_len
        seed = tracking.codebook_seed_ref(desc, ln, 1, min_len)
        cb, words, counts, stats = tracking.codebook_train_ref(desc, layout, ln, seed, 1, min_len)
        S, m = desc[member].astype(np.int64).sum(0), int(member.sum())
        assert m > 1 and np.array_equal(cb[0], (2 * S + m) // (2 * m))
        assert not words.any() and (counts == m).all() and (stats[0, :, 0] == m).all()


# ------------------------------------------------------------------ seeding
def test_seeding_without_a_length_array_draws_distinct_evenly_spread_slots():
    layout = _layout()
    desc = np.zeros((10, layout["dims"]), np.uint8)
    desc[:, 0] = np.arange(10)   # a row says which slot it came from
    assert tracking.codebook_seed_ref(desc, None, 5, 1)[:, 0].tolist() == [1, 3, 5, 7, 9]
    assert tracking.codebook_seed_ref(desc, None, 10, 1)[:, 0].tolist() == list(range(10))
    assert tracking.codebook_seed_ref(desc, None, 3, 1)[:, 0].tolist() == [1, 5, 8]   # floor(10 / 6), floor(30 / 6), floor(50 / 6)
    assert tracking.codebook_seed_ref(desc, None, 4, 7)[:, 0].tolist() == [1, 3, 6, 8]   # min_len without a length array: nothing
    many = tracking.codebook_seed_ref(desc, None, 25, 1)[:, 0]   # more words than slots: repeats, in order
    assert many.tolist() == [(2 * k + 1) * 10 // 50 for k in range(25)] and len(set(many.tolist())) == 10


def test_seeding_walks_to_the_next_member_and_wraps_around_the_end():
    layout = _layout()
    desc = np.zeros((10, layout["dims"]), np.uint8)
    desc[:, 0] = np.arange(10)
    desc[:, 1:] = 200 - np.arange(10)[:, None]   # the whole row travels, all four channels
    length = np.array([1, 1, 4, 1, 3, 1, 1, 2, 2, 1])
    cb = tracking.codebook_seed_ref(desc, length, 5, 3)          # members 2 and 4; s = 1, 3, 5, 7, 9
    assert cb[:, 0].tolist() == [2, 4, 2, 2, 2]                  # from 5 on: past the end and round to slot 2
    assert (cb[:, 1:] == 200 - cb[:, :1]).all()
    assert tracking.codebook_seed_ref(desc, length, 5, 4)[:, 0].tolist() == [2] * 5   # one member: every word
    assert tracking.codebook_seed_ref(desc, length, 2, 2)[:, 0].tolist() == [2, 7]    # s = 2, 7: members themselves


def test_seeding_without_a_member_is_all_zero():
    layout = _layout()
    desc = np.full((6, layout["dims"]), 77, np.uint8)
    assert not tracking.codebook_seed_ref(desc, np.ones(6, np.int32), 4, 2).any()
    assert not tracking.codebook_seed_ref(desc[:0], None, 4, 1).any()
    assert tracking.codebook_seed_ref(desc[:0], np.zeros(0, np.int32), 4, 1).shape == (4, layout["dims"])


# ------------------------------------------------------------------ the update
def test_a_words_entry_outside_the_codebook_belongs_to_no_word():
    layout = _layout(2, 3)
    _, _, _, desc, _ = _data(2, 3)
    desc = desc[:40]
    rng = np.random.default_rng(3)
    words = rng.integers(-2, 7, (40, 4))
    assert (words < 0).any() and (words >= 5).any()
    cb0 = rng.integers(0, 256, (5, layout["dims"])).astype(np.uint8)
    cb, counts = tracking.codebook_update_ref(desc, layout, words, None, cb0)
    inside = (words >= 0) & (words < 5)
    assert np.array_equal(counts.sum(1), inside.sum(0))
    kept = np.where(inside, words, 0)   # the same update with the outsiders taken out of the population per channel
    for c, seg in enumerate(tracking._channel_slices(layout)):
        only = inside[:, c]
        want, cnt = tracking.codebook_update_ref(desc[only], layout, kept[only], None, cb0)
        assert np.array_equal(cb[:, seg], want[:, seg]) and np.array_equal(counts[c], cnt[c])


def test_an_empty_word_keeps_its_bytes_and_a_filtered_slot_is_no_member():
    layout = _layout()
    desc = _rows([10, 20, 30, 41])
    words = np.array([[0, 0, 2, 2], [0, 2, 2, 0], [2, 2, 0, 0], [2, 0, 0, 2]], np.int32)
    cb0 = _rows([1, 2, 3])
    cb, counts = tracking.codebook_update_ref(desc, layout, words, None, cb0)
    assert (cb[1] == 2).all() and not counts[:, 1].any() and (counts[:, [0, 2]] == 2).all()
    segs = tracking._channel_slices(layout)
    assert (cb[0, segs[0]] == 15).all() and (cb[2, segs[0]] == 36).all()     # {10, 20} and {30, 41}: 35.5 -> 36
    assert (cb[0, segs[1]] == 26).all() and (cb[2, segs[1]] == 25).all()     # {10, 41}: 25.5 -> 26, {20, 30}
    length = np.array([3, 1, 3, 1])
    cb, counts = tracking.codebook_update_ref(desc, layout, words, length, cb0, 2)   # slots 0 and 2 alone
    assert (cb[0, segs[0]] == 10).all() and (cb[2, segs[0]] == 30).all() and (counts[:, [0, 2]] == 1).all()
    cb, counts = tracking.codebook_update_ref(desc, layout, words, length, cb0, 4)   # nobody: nothing moves
    assert np.array_equal(cb, cb0) and not counts.any()


@pytest.mark.parametrize("size", SIZES)
def test_the_update_does_not_depend_on_the_order_of_the_slots(size):
    layout, _, length, desc, codebook = _data(*size)
    words, _ = tracking.codebook_assign_ref(desc, layout, codebook[:16])
    want = tracking.codebook_update_ref(desc, layout, words, length, codebook[:16], 2)
    perm = np.random.default_rng(4).permutation(len(desc))
    got = tracking.codebook_update_ref(desc[perm], layout, words[perm], length[perm], codebook[:16], 2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (want[1] == 0).any() and (want[1] > 1).any() and not np.array_equal(want[0], codebook[:16])


# ------------------------------------------------------------------ training: the consequences
def _train(size, nwords, filtered, iters=8):
    layout, _, length, desc, _ = _data(*size)
    ln, min_len = (length, 3) if filtered else (None, 1)
    seed = tracking.codebook_seed_ref(desc, ln, nwords, min_len)
    return layout, desc, ln, min_len, seed, tracking.codebook_train_ref(desc, layout, ln, seed, iters, min_len)


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("nwords", [5, 16, 37])
@pytest.mark.parametrize("size", SIZES[:3])   # (at C = 27 eight rounds do not reach the fixed point)
def test_the_distortion_is_monotone_and_a_fixed_point_stays(size, nwords, filtered):
    layout, desc, ln, min_len, seed, (cb, words, counts, stats) = _train(size, nwords, filtered)
    member = np.ones(len(desc), bool) if ln is None else ln >= min_len
    assert (stats[0, :, 0] == member.sum()).all()
    assert (np.diff(stats[:, :, 1], axis=0) <= 0).all(), stats[:, :, 1]
    assert (counts.sum(1) == member.sum()).all()
    # the fixed point: the round after a round without changes reproduces words, counts and the channel's bytes
    for c, seg in enumerate(tracking._channel_slices(layout)):
        still = np.flatnonzero(stats[:, c, 0] == 0)
        assert len(still), (c, stats[:, c, 0])   # (8 rounds are enough on these data)
        t = int(still[0])
        assert not stats[t:, c, 0].any() and (stats[t:, c, 1] == stats[t, c, 1]).all()
        at_t = tracking.codebook_train_ref(desc, layout, ln, seed, t + 1, min_len)
        assert np.array_equal(at_t[0][:, seg], cb[:, seg]) and np.array_equal(at_t[2][c], counts[c])
        assert np.array_equal(at_t[1][member, c], words[member, c])


def test_one_case_moves_late_has_an_empty_word_and_strictly_improves():
    """the data are worth the tests above: a change in an iteration >= 2, an empty word, a strictly decreasing distortion"""
    _, _, _, _, _, (cb, words, counts, stats) = _train((2, 3), 16, False)
    assert stats[2:, :, 0].any() and (counts == 0).any()
    first_still = [int(np.flatnonzero(stats[:, c, 0] == 0)[0]) for c in range(4)]
    for c in range(4):   # strictly down in every round that still moved a member
        assert (np.diff(stats[:first_still[c], c, 1]) < 0).all(), (c, stats[:, c])
    assert max(first_still) >= 3


@pytest.mark.parametrize("filtered", [False, True])
def test_training_is_rounds_of_assignment_and_update(filtered):
    layout, desc, ln, min_len, seed, (cb, words, counts, stats) = _train((2, 3), 37, filtered, iters=3)
    member = np.ones(len(desc), bool) if ln is None else ln >= min_len
    step = seed
    for t in range(3):
        w, dist = tracking.codebook_assign_ref(desc, layout, step)
        assert np.array_equal(stats[t, :, 1], dist[member].astype(np.int64).sum(0))
        step, cnt = tracking.codebook_update_ref(desc, layout, w, ln, step, min_len)
    assert np.array_equal(step, cb) and np.array_equal(w, words) and np.array_equal(cnt, counts)
    again = tracking.codebook_assign_ref(desc, layout, cb)[0]   # the words of the returned codebook are another call
    assert again.shape == words.shape
    assert not np.shares_memory(cb, seed) and np.array_equal(seed, tracking.codebook_seed_ref(desc, ln, 37, min_len))
