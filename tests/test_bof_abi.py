"""CPU: the bag-of-features entry points (include/ofdis.h: ofdis_descriptor_normalize, ofdis_codebook_assign,
ofdis_bof_histogram, ofdis_track_bof) in the header, the binding and the export list, and the argument checks that return before
any device work.  Host buffers stand in for the device arrays: every call here returns before it would launch.  The kernels:
tests/test_gpu_bof.py."""
import re

import numpy as np
import pytest

import abi
from of_dis_amd import capi

_p = abi.ptr


def test_the_bounds_the_header_derives():
    assert 1152 * 255 * 255 < 2 ** 31 and 511 * 511 * 1152 * (2 ** 32 - 1) < 2 ** 62  # the header's two bounds


def test_the_header_states_the_definition_and_its_consequences():
    section = abi.section("Bag-of-features encoding of those descriptors", "int ofdis_track_bof")
    for words in ("Identity:", "Known value:", "Ties:", "Sums:", "Contract independence:", "Not provided:", "k-means", "Fisher vectors",
                  "shape channel", "static tracks", "relies on no memset", r"q\*q\*S <= 510\*510\*h_e", "bit-identical",
                  "smallest k that attains the minimum", r"floor\(sqrt\(floor\(510\*510\*h_e / S\)\)\)", "normalize_descriptors_u8",
                  "codebook_assign_ref", "bof_ref"):
        assert re.search(words, section), words
    desc = abi.section("Trajectory-aligned descriptors of dense tracks", "int ofdis_track_descriptors")
    assert "ofdis_track_bof" in desc[desc.index("Not provided:"):]  # the descriptor section points here


# ------------------------------------------------------------------ argument checks
class _Host:
    """host stand-ins for 64 slots of a 2x2x2 descriptor and a codebook of 5 words"""

    def __init__(self):
        D = 33 * 8
        self.hist, self.desc = np.zeros((64, D), np.uint32), np.zeros((64, D), np.uint8)
        self.len, self.info = np.ones(64, np.int32), np.zeros(2, np.int64)
        self.codebook = np.zeros((5, D), np.uint8)
        self.words, self.dist, self.bof = np.zeros((64, 4), np.int32), np.zeros((64, 4), np.int32), np.zeros((4, 5), np.uint32)


def _normalize(hb, hist=True, info=True, max_tracks=64, nxy=2, nt=2, desc=True, **_):
    return capi.lib().ofdis_descriptor_normalize(_p(hb.hist, hist), _p(hb.info, info), max_tracks, nxy, nt, _p(hb.desc, desc), None)


def _assign(hb, desc=True, info=True, max_tracks=64, nxy=2, nt=2, codebook=True, nwords=5, words=True, dist=True, **_):
    return capi.lib().ofdis_codebook_assign(_p(hb.desc, desc), _p(hb.info, info), max_tracks, nxy, nt, _p(hb.codebook, codebook),
                                            nwords, _p(hb.words, words), _p(hb.dist, dist), None)


def _histogram(hb, words=True, length=True, info=True, max_tracks=64, nwords=5, min_len=1, bof=True, **_):
    return capi.lib().ofdis_bof_histogram(_p(hb.words, words), _p(hb.len, length), _p(hb.info, info), max_tracks, nwords, min_len,
                                          _p(hb.bof, bof), None)


def _fused(hb, hist=True, length=True, info=True, max_tracks=64, nxy=2, nt=2, codebook=True, nwords=5, min_len=1, bof=True,
           words=True, **_):
    return capi.lib().ofdis_track_bof(_p(hb.hist, hist), _p(hb.len, length), _p(hb.info, info), max_tracks, nxy, nt,
                                      _p(hb.codebook, codebook), nwords, min_len, _p(hb.bof, bof), _p(hb.words, words), None)


CALLS = {"normalize": _normalize, "assign": _assign, "histogram": _histogram, "fused": _fused}
REQUIRED = {"normalize": ["hist", "info", "desc"], "assign": ["desc", "info", "codebook", "words"],
            "histogram": ["words", "length", "info", "bof"], "fused": ["hist", "length", "info", "codebook", "bof"]}
VALUES = {"normalize": ["max_tracks", "nxy", "nt"], "assign": ["max_tracks", "nxy", "nt", "nwords"],
          "histogram": ["max_tracks", "nwords", "min_len"], "fused": ["max_tracks", "nxy", "nt", "nwords", "min_len"]}
BAD = {"max_tracks": [0, -1, (1 << 24) + 1], "nxy": [0, -1, 5], "nt": [0, -1, 9], "nwords": [0, -1, 16385], "min_len": [0, -1]}
ENDS = {"max_tracks": [1, 1 << 24], "nxy": [1, 4], "nt": [1, 8], "nwords": [1, 16384], "min_len": [1, 2 ** 31 - 1]}


@pytest.mark.parametrize("call,which", [(c, w) for c, ws in REQUIRED.items() for w in ws])
def test_rejects_null_pointers(call, which):
    abi.rejected(CALLS[call](_Host(), **{which: False}), {"length": "len"}.get(which, which))


@pytest.mark.parametrize("call,name,value", [(c, n, v) for c, ns in VALUES.items() for n in ns for v in BAD[n]])
def test_rejects_values_outside_their_ranges(call, name, value):
    abi.rejected(CALLS[call](_Host(), **{name: value}), name)


@pytest.mark.parametrize("call", list(CALLS))
def test_the_value_checks_accept_their_closed_ranges(call):
    """both ends of every range pass their check: each is paired with a bad value of the argument checked right after it, and
    the call fails naming that one -- an earlier failure would name another argument.  The last argument of each call has
    nothing after it: a call with all of them right would launch, so its accepted values are exercised on the device
    (tests/test_gpu_bof.py)."""
    hb = _Host()
    names = VALUES[call]
    for at, name in enumerate(names[:-1]):
        later = names[at + 1]
        for v in ENDS[name]:
            abi.rejected(CALLS[call](hb, **{name: v, later: BAD[later][0]}), later)
    # the optional pointers may be NULL: the call passes them and fails at the last value check
    last = names[-1]
    optional = {"assign": "dist", "fused": "words"}.get(call)
    if optional:
        abi.rejected(CALLS[call](hb, **{optional: False, last: BAD[last][0]}), last)
