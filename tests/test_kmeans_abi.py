"""CPU: the codebook-training entry points (include/ofdis.h: ofdis_codebook_train_work_bytes, ofdis_codebook_seed,
ofdis_codebook_update, ofdis_codebook_train) in the header, the binding and the export list, and the argument checks that return
before any device work.  Host buffers stand in for the device arrays: every call here returns before it would launch.  The
model: tests/test_kmeans_ref.py; the kernels: tests/test_gpu_kmeans.py."""
import re

import numpy as np
import pytest

import abi
from of_dis_amd import capi

_p = abi.ptr


def test_the_bounds_the_header_derives():
    assert 2 ** 24 * 255 < 2 ** 32 and 2 ** 24 * 1152 * 255 * 255 < 2 ** 55   # the header's two bounds


def test_the_header_states_the_definition_and_its_consequences():
    hdr = abi.header()
    section = abi.section("K-means training of the bag-of-features codebook", "int ofdis_codebook_train(")
    assert hdr.index("int ofdis_track_bof") < hdr.index("K-means training of the bag-of-features codebook")   # its own section, after
    for words in ("Members\\.", "Seeding \\(ofdis_codebook_seed\\)", "Update \\(ofdis_codebook_update\\)",
                  "Training \\(ofdis_codebook_train\\)", r"s_k = floor\(\(2k\+1\)\*n / \(2\*nwords\)\)", "cyclically",
                  r"floor\(\(2\*S_e \+ \|M\|\) / \(2\*\|M\|\)\)", "rounded half up", "keeps its bytes", "belongs to no word",
                  "relies on no memset", "Monotone:", "Fixed point:", "Order:", "Route:", "Contract independence:", "Known values:",
                  "bit-identical", r"members \{0, 1\} give 1", r"\{0, 0, 1\} give 0", r"\{254, 255\} give 255", "Not provided:",
                  "re-seeding of empty words", r"k-means\+\+", "subsampling", "early exit", "Fisher vectors", "shape channel",
                  "OFDIS_KMEANS_MAX_ITERS", "before the last update", "codebook_seed_ref", "codebook_update_ref", "codebook_train_ref"):
        assert re.search(words, section), words
    bof = abi.section("Bag-of-features encoding of those descriptors", "int ofdis_track_bof")
    assert "ofdis_codebook_train" in bof[bof.index("Not provided:"):]   # the bag-of-features section points here


# ------------------------------------------------------------------ argument checks
MAX_TRACKS, NXY, NT, NWORDS = 64, 2, 2, 5


def _need(max_tracks=MAX_TRACKS, nxy=NXY, nt=NT, nwords=NWORDS):
    return capi.lib().ofdis_codebook_train_work_bytes(max_tracks, nxy, nt, nwords)


class _Host:
    """host stand-ins for 64 slots of a 2x2x2 descriptor, a codebook of 5 words and the work buffer"""

    def __init__(self):
        D = 33 * 8
        self.desc, self.words = np.zeros((MAX_TRACKS, D), np.uint8), np.zeros((MAX_TRACKS, 4), np.int32)
        self.len, self.info = np.ones(MAX_TRACKS, np.int32), np.zeros(2, np.int64)
        self.codebook, self.counts = np.zeros((NWORDS, D), np.uint8), np.zeros((4, NWORDS), np.uint32)
        self.stats = np.zeros((capi.KMEANS_MAX_ITERS, 4, 2), np.int64)
        self.work = np.zeros(_need() // 8 + 2, np.int64)   # 8-byte aligned, a little more than needed


def _work(hb, work, work_bytes):
    """(pointer, bytes) of the work argument: True = the buffer as it should be, False = NULL, an int = that many bytes off"""
    ptr = None if work is False else hb.work.ctypes.data + (0 if work is True else work)
    return ptr, _need() if work_bytes is None else work_bytes


def _seed(hb, desc=True, length=True, info=True, max_tracks=MAX_TRACKS, nxy=NXY, nt=NT, nwords=NWORDS, min_len=1, codebook=True, **_):
    return capi.lib().ofdis_codebook_seed(_p(hb.desc, desc), _p(hb.len, length), _p(hb.info, info), max_tracks, nxy, nt, nwords,
                                          min_len, _p(hb.codebook, codebook), None)


def _update(hb, desc=True, words=True, length=True, info=True, max_tracks=MAX_TRACKS, nxy=NXY, nt=NT, nwords=NWORDS, min_len=1,
            codebook=True, counts=True, work=True, work_bytes=None, **_):
    ptr, nbytes = _work(hb, work, work_bytes)
    return capi.lib().ofdis_codebook_update(_p(hb.desc, desc), _p(hb.words, words), _p(hb.len, length), _p(hb.info, info), max_tracks,
                                            nxy, nt, nwords, min_len, _p(hb.codebook, codebook), _p(hb.counts, counts), ptr, nbytes,
                                            None)


def _train(hb, desc=True, length=True, info=True, max_tracks=MAX_TRACKS, nxy=NXY, nt=NT, nwords=NWORDS, min_len=1, iters=3,
           codebook=True, words=True, counts=True, stats=True, work=True, work_bytes=None, **_):
    ptr, nbytes = _work(hb, work, work_bytes)
    return capi.lib().ofdis_codebook_train(_p(hb.desc, desc), _p(hb.len, length), _p(hb.info, info), max_tracks, nxy, nt, nwords,
                                           min_len, iters, _p(hb.codebook, codebook), _p(hb.words, words), _p(hb.counts, counts),
                                           _p(hb.stats, stats), ptr, nbytes, None)


CALLS = {"seed": _seed, "update": _update, "train": _train}
REQUIRED = {"seed": ["desc", "info", "codebook"], "update": ["desc", "words", "info", "codebook", "counts", "work"],
            "train": ["desc", "info", "codebook", "words", "counts", "work"]}
OPTIONAL = {"seed": ["length"], "update": ["length"], "train": ["length", "stats"]}
# in the order the calls check them
VALUES = {"seed": ["max_tracks", "nxy", "nt", "nwords", "min_len"], "update": ["max_tracks", "nxy", "nt", "nwords", "min_len"],
          "train": ["max_tracks", "nxy", "nt", "nwords", "min_len", "iters"]}
BAD = {"max_tracks": [0, -1, (1 << 24) + 1], "nxy": [0, -1, 5], "nt": [0, -1, 9], "nwords": [0, -1, 16385], "min_len": [0, -1],
       "iters": [0, -1, 1001]}
ENDS = {"max_tracks": [1, 1 << 24], "nxy": [1, 4], "nt": [1, 8], "nwords": [1, 16384], "min_len": [1, 2 ** 31 - 1], "iters": [1, 1000]}


@pytest.mark.parametrize("call,which", [(c, w) for c, ws in REQUIRED.items() for w in ws])
def test_rejects_null_pointers(call, which):
    abi.rejected(CALLS[call](_Host(), **{which: False}), which)


@pytest.mark.parametrize("call,name,value", [(c, n, v) for c, ns in VALUES.items() for n in ns for v in BAD[n]])
def test_rejects_values_outside_their_ranges(call, name, value):
    abi.rejected(CALLS[call](_Host(), **{name: value}), name)


@pytest.mark.parametrize("call", list(CALLS))
def test_the_value_checks_accept_their_closed_ranges(call):
    """both ends of every range pass their check: each is paired with a bad value of the argument checked right after it, and
    the call fails naming that one -- an earlier failure would name another argument.  The last value of ofdis_codebook_update
    and ofdis_codebook_train is followed by the work buffer, which is then too small by a byte; the last one of
    ofdis_codebook_seed has nothing after it: a call with all of them right would launch, so its accepted values are exercised
    on the device (tests/test_gpu_kmeans.py)."""
    hb = _Host()
    names = VALUES[call]
    for at, name in enumerate(names[:-1]):
        later = names[at + 1]
        for v in ENDS[name]:
            abi.rejected(CALLS[call](hb, **{name: v, later: BAD[later][0]}), later)
    if call != "seed":
        for v in ENDS[names[-1]]:
            abi.rejected(CALLS[call](hb, **{names[-1]: v, "work_bytes": _need() - 1}), "work")


@pytest.mark.parametrize("call", list(CALLS))
def test_the_optional_pointers_may_be_null(call):
    """len and stats: the call passes them and fails at the last check, which names something else"""
    hb = _Host()
    last = VALUES[call][-1]
    for optional in OPTIONAL[call]:
        abi.rejected(CALLS[call](hb, **{optional: False, last: BAD[last][0]}), last)
        if call != "seed":
            abi.rejected(CALLS[call](hb, **{optional: False, "work_bytes": _need() - 1}), "work")


@pytest.mark.parametrize("call", ["update", "train"])
def test_rejects_a_small_or_misaligned_work_buffer(call):
    hb = _Host()
    for nbytes in (0, 8, _need() - 8, _need() - 1):
        abi.rejected(CALLS[call](hb, work_bytes=nbytes), "work")
    for shift in (1, 2, 4, 7):   # enough bytes behind it, but not on a multiple of 8
        abi.rejected(CALLS[call](hb, work=shift, work_bytes=_need()), "aligned")
    # the size is that of the call's own max_tracks and nwords, not of some other
    abi.rejected(CALLS[call](hb, max_tracks=MAX_TRACKS + 1000, work_bytes=_need()), "work")


def test_the_work_bytes_are_zero_for_rejected_sizes_and_grow_with_the_sizes():
    for name in ("max_tracks", "nxy", "nt", "nwords"):
        for v in BAD[name]:
            assert _need(**{name: v}) == 0, (name, v)
        for v in ENDS[name]:
            assert _need(**{name: v}) > 0 and _need(**{name: v}) % 8 == 0, (name, v)
    assert _need(max_tracks=1 << 24, nxy=4, nt=8, nwords=16384) > 2 ** 31   # size_t, not int
    assert _need(max_tracks=2000) > _need(max_tracks=1000) > 64 * 1000      # prev, dist, rank and order: 16 bytes per slot each
    assert _need(nwords=16384) > _need(nwords=1) and _need(nxy=4, nt=8) > _need(nxy=1, nt=1)
    assert capi.codebook_train_work_bytes(MAX_TRACKS, NXY, NT, NWORDS) == _need()
