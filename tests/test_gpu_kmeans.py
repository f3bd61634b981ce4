"""-m gpu: the k-means training of the codebook (include/ofdis.h: ofdis_codebook_seed, ofdis_codebook_update,
ofdis_codebook_train) against of_dis_amd/tracking.py (codebook_seed_ref, codebook_update_ref, codebook_train_ref), every
comparison by integer equality.

The descriptors are the model's normalisation of the synthetic hist rows of tests/test_gpu_bof.py (no flow run): a case takes
the first ntracks rows.  The model runs four rounds once per case and keeps every round, so the cases of one and four iterations,
the chain of single calls and the update alone share it.  The conditions on the data (late changes, empty words, improving
distortion) are asserted on the model: tests/test_kmeans_ref.py."""
import functools

import numpy as np
import pytest

from of_dis_amd import tracking
from test_gpu_bof import END_TO_END_16_CELLS, NEW_LAYOUTS, _data, _id, _padded
from test_gpu_descriptors import CASES as DESC_CASES, MIN_FLOW, _case as _desc_case

pytestmark = pytest.mark.gpu
# channels of 8/9, 96/108 and 1024/1152 bytes, C = 1, 12 and 128: the sum with 4 and 32 lanes in one pass and with 64 lanes in five
# passes over all 288 dwords; the assignment kernels <2, 8> (twice) and <18, 1>.  The other 25 values of C: NEW_LAYOUTS
LAYOUTS = [(1, 1), (2, 3), (4, 8)]
NWORDS = [1, 5, 37, 300]             # one word owns everything; below and above the 16 words of an MFMA; more words than tracks
NTRACKS = [1, 17, 200]
SWEEP_CASES = [(5, 200), (37, 17)]   # (nwords, ntracks) of the layouts of NEW_LAYOUTS
# segments longer than a chunk (700 slots): with LAYOUTS a layout of every class of the sum that occurs -- the lanes, the passes,
# the passes either channel fills and whether its last one is cut, 9 C mod 4 -- and of every pair of thread splits of the finish
# kernel (tests/test_descriptor_layout_classes.py holds the list to that).  C = 2 .. 7, 9, 16, 18, 27, 32, 36, 45, 54, 63, 64, 72,
# 96, 112
LONG_SEGMENT_LAYOUTS = [(1, 2), (1, 3), (1, 4), (1, 5), (1, 6), (1, 7), (3, 1), (4, 1), (3, 2), (3, 3), (2, 8), (3, 4), (3, 5), (3, 6),
                        (3, 7), (4, 4), (3, 8), (4, 6), (4, 7)]
TAIL_BYTES_LAYOUTS = [(1, 2), (3, 3)]   # 9 C mod 4 = 2 and 3: a channel whose last dword is cut, two and three bytes of it written
MIN_LEN = 3                          # with the length array; without it every slot is a member
ROUNDS = 4
GUARD = 256
FILL = 0xAB


@functools.lru_cache(maxsize=None)
def _model(nxy, nt, nwords, ntracks, filtered, repeat=1):
    """(layout, desc, length or None, min_len, seed, rounds, stats): rounds[t] = (codebook after round t, words, dist, counts of
    round t), stats [ROUNDS][4][2]; repeat: the rows taken that many times over (more members than one chunk of the sum)"""
    layout, _, length, desc, _ = _data(nxy, nt)
    desc, length = np.tile(desc[:ntracks], (repeat, 1)), np.tile(length[:ntracks], repeat)
    if repeat > 1:   # not the same row again: the later copies move a little
        desc = np.clip(desc.astype(int) + (np.arange(len(desc)) // ntracks)[:, None] * 3, 0, 255).astype(np.uint8)
    ln, min_len = (length, MIN_LEN) if filtered else (None, 1)
    member = np.ones(len(desc), bool) if ln is None else ln >= min_len
    seed = tracking.codebook_seed_ref(desc, ln, nwords, min_len)
    rounds, stats, cb, before = [], np.zeros((ROUNDS, 4, 2), np.int64), seed, None
    for t in range(ROUNDS):
        words, dist = tracking.codebook_assign_ref(desc, layout, cb)
        changed = np.ones(words.shape, bool) if before is None else words != before
        stats[t, :, 0], stats[t, :, 1] = (changed & member[:, None]).sum(0), dist[member].astype(np.int64).sum(0)
        cb, counts = tracking.codebook_update_ref(desc, layout, words, ln, cb, min_len)
        rounds.append((cb, words, dist, counts))
        before = words
    return layout, desc, ln, min_len, seed, rounds, stats


class _Dev:
    """the device side of one case: max_tracks = ntracks + idle slots; every output and the work buffer pre-filled"""

    def __init__(self, gpu, nxy, nt, desc, ln, nwords, idle=9, info0=None, fill=FILL, stream=None):
        self.gpu, self.args, self.nwords, self.fill, self.stream = gpu, (nxy, nt), nwords, fill, stream
        self.n, self.D = desc.shape
        self.slots = self.n + idle
        pad = _padded if idle else (lambda a: a)
        self.dd = gpu.Dev(pad(desc))
        self.dl = gpu.Dev(pad(np.ascontiguousarray(ln, np.int32))) if ln is not None else None
        self.info = np.array([self.n if info0 is None else info0, 7], np.int64)
        self.di = gpu.Dev(self.info)
        self.work_bytes = gpu.codebook_train_work_bytes(self.slots, nxy, nt, nwords)
        assert self.work_bytes > 0
        self.sizes = dict(codebook=nwords * self.D, words=self.slots * 16, counts=16 * nwords, stats=ROUNDS * 64, work=self.work_bytes)
        self.dev = {}

    def s(self):
        return self.stream.ptr if self.stream else None

    def buf(self, key, init=None, fill=None):
        """a fresh pre-filled buffer for output `key` with its guard; init: the bytes it starts with (the in/out codebook)"""
        a = np.full(self.sizes[key] + GUARD, self.fill if fill is None else fill, np.uint8)
        if init is not None:
            a[:self.sizes[key]] = np.ascontiguousarray(init).view(np.uint8).ravel()
        self.dev[key] = self.gpu.Dev(a)
        return self.dev[key].ptr

    def lp(self):
        return self.dl.ptr if self.dl else None

    def seed(self, min_len):
        nxy, nt = self.args
        self.gpu.check(self.gpu.lib().ofdis_codebook_seed(self.dd.ptr, self.lp(), self.di.ptr, self.slots, nxy, nt, self.nwords, min_len,
                                                          self.buf("codebook"), self.s()))
        return self.fetch(("codebook",))["codebook"]

    def train(self, cb0, min_len, iters, stats=True):
        nxy, nt = self.args
        self.gpu.codebook_train_dev(self.dd.ptr, self.lp(), self.di.ptr, self.slots, nxy, nt, self.nwords, min_len, iters,
                                    self.buf("codebook", cb0), self.buf("words"), self.buf("counts"),
                                    self.buf("stats") if stats else None, self.buf("work"), self.work_bytes, self.s())
        return self.fetch(("codebook", "words", "counts") + (("stats",) if stats else ()))

    def chain(self, cb0, min_len, iters):
        """iters x (ofdis_codebook_assign + ofdis_codebook_update); the codebook after every round"""
        nxy, nt = self.args
        L, after = self.gpu.lib(), []
        pc, pw, pn, pk = self.buf("codebook", cb0), self.buf("words"), self.buf("counts"), self.buf("work")
        for _ in range(iters):
            self.gpu.check(L.ofdis_codebook_assign(self.dd.ptr, self.di.ptr, self.slots, nxy, nt, pc, self.nwords, pw, None, self.s()))
            self.gpu.check(L.ofdis_codebook_update(self.dd.ptr, pw, self.lp(), self.di.ptr, self.slots, nxy, nt, self.nwords, min_len,
                                                   pc, pn, pk, self.work_bytes, self.s()))
            after.append(self.fetch(("codebook", "words", "counts")))
        return after

    def fetch(self, keys):
        """the outputs as arrays; the guards behind them, the idle slots of words and info are as they were"""
        self.gpu.check(self.gpu.lib().ofdis_sync(self.s()))
        out = {}
        for k in keys:
            v = self.sizes[k]
            raw = self.dev[k].get((v + GUARD,), np.uint8)
            assert (raw[v:] == self.fill).all(), f"guard behind {k}"
            out[k] = raw[:v]
        if "codebook" in out:
            out["codebook"] = out["codebook"].reshape(self.nwords, self.D)
        if "words" in out:
            w = out["words"].view(np.int32).reshape(self.slots, 4)
            live = min(max(int(self.info[0]), 0), self.slots)
            assert (w[live:].view(np.uint8) == self.fill).all(), "idle slots of words"
            out["words"] = w[:live]
        if "counts" in out:
            out["counts"] = out["counts"].view(np.uint32).reshape(4, self.nwords)
        if "stats" in out:
            out["stats"] = out["stats"].view(np.int64).reshape(ROUNDS, 4, 2)
        assert np.array_equal(self.di.get((2,), np.int64), self.info)   # the inputs are inputs
        return out


def _same(got, want, what):
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:3], got[got != want][:3], want[got != want][:3])


def _check_train(got, rounds, stats, iters, what, with_stats=True):
    cb, words, _, counts = rounds[iters - 1]
    _same(got["codebook"], cb, (what, "codebook"))
    _same(got["words"], words, (what, "words"))
    _same(got["counts"], counts, (what, "counts"))
    if with_stats:
        _same(got["stats"][:iters], stats[:iters], (what, "stats"))
        assert (got["stats"][iters:].view(np.uint8) == FILL).all(), (what, "stats of rounds never run")


# ------------------------------------------------------------------ 1. seed, update and train against the model; train against the chain
@pytest.mark.parametrize("ntracks", NTRACKS)
@pytest.mark.parametrize("nwords", NWORDS)
@pytest.mark.parametrize("size", LAYOUTS, ids=lambda s: f"{s[0]}x{s[0]}x{s[1]}")
def test_the_calls_match_the_model(gpu, size, nwords, ntracks):
    _calls_match_the_model(gpu, size, nwords, ntracks)


@pytest.mark.parametrize("case", SWEEP_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
@pytest.mark.parametrize("size", NEW_LAYOUTS, ids=_id)
def test_the_calls_match_the_model_at_every_layout(gpu, size, case):
    _calls_match_the_model(gpu, size, *case)


def _calls_match_the_model(gpu, size, nwords, ntracks):
    nxy, nt = size
    for filtered in (False, True):
        layout, desc, ln, min_len, seed, rounds, stats = _model(nxy, nt, nwords, ntracks, filtered)
        what = (size, nwords, ntracks, filtered)
        dev = _Dev(gpu, nxy, nt, desc, ln, nwords)
        _same(dev.seed(min_len), seed, (what, "seed"))
        chain = dev.chain(seed, min_len, ROUNDS)
        for t, got in enumerate(chain):   # ofdis_codebook_update alone, round by round
            _check_train(got, rounds, stats, t + 1, (what, "chain", t), with_stats=False)
        for iters in (1, ROUNDS):
            got = dev.train(seed, min_len, iters)
            _check_train(got, rounds, stats, iters, (what, "train", iters))
            for k in ("codebook", "words", "counts"):   # the fused route is the chain
                _same(got[k], chain[iters - 1][k], (what, "route", iters, k))
            bare = dev.train(seed, min_len, iters, stats=False)
            for k in ("codebook", "words", "counts"):
                _same(bare[k], got[k], (what, "stats == NULL", iters, k))


# ------------------------------------------------------------------ 2. segments longer than one chunk of the sum
@pytest.mark.parametrize("nwords", [1, 5])
@pytest.mark.parametrize("size", LAYOUTS + LONG_SEGMENT_LAYOUTS, ids=_id)
def test_words_with_more_members_than_one_wavefront_sums(gpu, size, nwords):
    """700 slots: with one word its segment spans three chunks of 256 (a head, a middle and a tail part), with five the segments
    straddle the chunk borders; every part goes through the slab and the last launch"""
    nxy, nt = size
    for filtered in (False, True):
        layout, desc, ln, min_len, seed, rounds, stats = _model(nxy, nt, nwords, 175, filtered, 4)
        members = len(desc) if ln is None else int((ln >= min_len).sum())
        assert len(desc) == 700 and members > (256 if filtered else 512), members   # two chunks, three chunks
        dev = _Dev(gpu, nxy, nt, desc, ln, nwords)
        _same(dev.seed(min_len), seed, (size, nwords, filtered, "seed"))
        for iters in (1, ROUNDS):
            _check_train(dev.train(seed, min_len, iters), rounds, stats, iters, (size, nwords, filtered, iters))


# ------------------------------------------------------------------ 3. ntracks on the device: none, and more than the slots
@pytest.mark.parametrize("size", LAYOUTS, ids=lambda s: f"{s[0]}x{s[0]}x{s[1]}")
def test_no_tracks_at_all(gpu, size):
    nxy, nt = size
    layout, desc, ln, min_len, seed, _, _ = _model(nxy, nt, 5, 17, True)
    dev = _Dev(gpu, nxy, nt, desc, ln, 5, info0=0)
    assert not dev.seed(min_len).any()
    got = dev.train(seed, min_len, 2)
    _same(got["codebook"], seed, "codebook")
    assert got["words"].shape == (0, 4) and not got["counts"].any() and not got["stats"][:2].any()
    got = dev.chain(seed, min_len, 1)[0]
    _same(got["codebook"], seed, "codebook")
    assert not got["counts"].any()


@pytest.mark.parametrize("size", LAYOUTS, ids=lambda s: f"{s[0]}x{s[0]}x{s[1]}")
def test_more_tracks_than_slots_are_clamped(gpu, size):
    nxy, nt = size
    layout, desc, ln, min_len, seed, rounds, stats = _model(nxy, nt, 37, 200, True)
    dev = _Dev(gpu, nxy, nt, desc, ln, 37, idle=0, info0=200 + 1000)
    _same(dev.seed(min_len), seed, "seed")
    _check_train(dev.train(seed, min_len, ROUNDS), rounds, stats, ROUNDS, "clamped")


def test_no_member_at_all(gpu):
    """tracks, but none long enough: a zero seed, nothing moves, every count zero, the distances not summed"""
    layout, desc, ln, _, seed, _, _ = _model(2, 3, 5, 17, True)
    dev = _Dev(gpu, 2, 3, desc, ln, 5)
    assert not dev.seed(100).any()
    got = dev.train(seed, 100, 2)
    _same(got["codebook"], seed, "codebook")
    _same(got["words"], tracking.codebook_assign_ref(desc, layout, seed)[0], "words")   # assigned all the same
    assert not got["counts"].any() and not got["stats"][:2].any()


# ------------------------------------------------------------------ 4. a words array of the caller
@pytest.mark.parametrize("size", LAYOUTS + TAIL_BYTES_LAYOUTS, ids=_id)
def test_a_words_array_of_the_caller_with_entries_outside_the_codebook(gpu, size):
    nxy, nt = size
    layout, _, length, desc, codebook = _data(nxy, nt)
    rng = np.random.default_rng(8)
    words = rng.integers(-3, 12, (len(desc), 4)).astype(np.int32)
    words[words == 4] = 20   # word 4 stays empty
    words[::7] = [2 ** 31 - 1, -2 ** 31, 9, -1]
    for ln, min_len in ((None, 1), (length, 3)):
        want = tracking.codebook_update_ref(desc, layout, words, ln, codebook[:9], min_len)
        got = gpu.codebook_update(desc, words, codebook[:9], nxy, nt, ln, min_len)
        _same(got[0], want[0], "codebook"), _same(got[1], want[1], "counts")
        assert not want[1][:, 4].any() and np.array_equal(want[0][4], codebook[4]) and 0 < want[1].sum() < 4 * len(desc)


def test_the_host_wrappers(gpu):
    layout, desc, ln, min_len, seed, rounds, stats = _model(2, 3, 37, 200, True)
    _same(gpu.codebook_seed(desc, 2, 3, 37, ln, min_len), seed, "seed")
    got = gpu.codebook_train(desc, seed, 2, 3, ROUNDS, ln, min_len)
    for a, b, k in zip(got, (rounds[-1][0], rounds[-1][1], rounds[-1][3], stats), ("codebook", "words", "counts", "stats")):
        _same(a, b, k)
    none = gpu.codebook_train(desc[:0], seed, 2, 3, 1)
    assert np.array_equal(none[0], seed) and none[1].shape == (0, 4) and not none[2].any() and not none[3].any()


# ------------------------------------------------------------------ 5. determinism and purity
def test_twice_the_same_bytes_on_a_stream_of_its_own(gpu):
    """ofdis_codebook_train twice on a non-default stream, into outputs and a work buffer pre-filled with different garbage: the
    same bytes, and the model's"""
    nxy, nt, nwords = 2, 3, 37
    layout, desc, ln, min_len, seed, rounds, stats = _model(nxy, nt, nwords, 200, True)
    stream = gpu.Stream()
    try:
        first = _Dev(gpu, nxy, nt, desc, ln, nwords, stream=stream).train(seed, min_len, ROUNDS)
        again = _Dev(gpu, nxy, nt, desc, ln, nwords, fill=0x5C, stream=stream).train(seed, min_len, ROUNDS)
        _check_train(first, rounds, stats, ROUNDS, "stream")
        for k in first:
            _same(again[k], first[k], k)
    finally:
        stream.close()


# ------------------------------------------------------------------ 6. end to end behind ofdis_track_descriptors
def test_end_to_end_behind_the_descriptors(gpu):
    """hist of the device -> normalise -> seed -> train 3 rounds -> ofdis_track_bof with the trained codebook, against bof_ref on
    the model's codebook"""
    _end_to_end(gpu, min(DESC_CASES, key=lambda c: c[0] * c[1]))   # the smallest gray case of tests/test_gpu_descriptors.py


def test_end_to_end_behind_the_descriptors_of_16_cells(gpu):
    """the same at N 64, nxy 4, nt 1 (C = 16): the sum with 64 lanes in one pass, the finish split 128 and 256, and the device's
    own hist through bof_assign_kernel<6, 3, true>"""
    _end_to_end(gpu, END_TO_END_16_CELLS)


def _end_to_end(gpu, case):
    w, h, _, _, npairs, _, N, nxy, nt = case
    frames, fw, (tracks, start, length, info), want, _ = _desc_case(*case, 1)
    n, lmax = len(length), tracks.shape[0] - 1
    layout = tracking.descriptor_layout(N, nxy, nt)
    D, nwords, iters = layout["dims"], 4, 3
    desc = tracking.normalize_descriptors_u8(want[0], layout)   # the model's own hist
    assert n > nwords and (length >= 2).any() and (length < 2).any() and want[0].any(), np.bincount(length)
    L = gpu.lib()
    dfr, dfw, dt, ds, dl, di = (gpu.Dev(a) for a in (frames, fw, tracks, start, length, info))
    work = gpu.Dev(nbytes=gpu.codebook_train_work_bytes(n, nxy, nt, nwords))
    for min_len in (1, 2):   # every track; the tracks that moved at least once (a track of one point has a zero hist)
        cb, _, _, stats = tracking.codebook_train_ref(desc, layout, length, tracking.codebook_seed_ref(desc, length, nwords, min_len),
                                                      iters, min_len)
        words, _ = tracking.codebook_assign_ref(desc, layout, cb)
        dh, dd, dc, dw, dn, dst, db, dbw = (gpu.Dev(np.full(b, FILL, np.uint8)) for b in
                                            (n * D * 4, n * D, nwords * D, n * 16, 16 * nwords, iters * 64, 16 * nwords, n * 16))
        gpu.track_descriptors_dev(dfr.ptr, dfw.ptr, npairs, w, h, 1, dt.ptr, ds.ptr, dl.ptr, di.ptr, lmax, n, N, nxy, nt, MIN_FLOW, dh.ptr)
        gpu.check(L.ofdis_descriptor_normalize(dh.ptr, di.ptr, n, nxy, nt, dd.ptr, None))
        gpu.check(L.ofdis_codebook_seed(dd.ptr, dl.ptr, di.ptr, n, nxy, nt, nwords, min_len, dc.ptr, None))
        gpu.codebook_train_dev(dd.ptr, dl.ptr, di.ptr, n, nxy, nt, nwords, min_len, iters, dc.ptr, dw.ptr, dn.ptr, dst.ptr, work.ptr,
                               work.nbytes)
        gpu.track_bof_dev(dh.ptr, dl.ptr, di.ptr, n, nxy, nt, dc.ptr, nwords, min_len, db.ptr, dbw.ptr)
        gpu.check(L.ofdis_sync(None))
        _same(dc.get((nwords, D), np.uint8), cb, "codebook")
        _same(dst.get((iters, 4, 2), np.int64), stats, "stats")
        _same(dbw.get((n, 4), np.int32), words, "words")
        _same(db.get((4, nwords), np.uint32), tracking.bof_ref(words, length, nwords, min_len), "bof")
