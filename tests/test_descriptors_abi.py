"""CPU: the descriptor entry points (include/ofdis.h: ofdis_track_descriptor_dims, ofdis_track_descriptors) in the header, the
binding and the export list, and the argument checks that return before any device work.  Host buffers stand in for the device
arrays: every call here returns before it would launch.  The kernel: tests/test_gpu_descriptors.py."""
import math
import re

import numpy as np
import pytest

import abi
from of_dis_amd import capi, tracking

_f32 = np.float32
_p = abi.ptr


def test_the_channels_have_33_bins():
    assert sum(bins for _, bins, _ in tracking.DESC_CHANNELS) == 33


def test_the_header_states_the_definition_and_its_consequences():
    section = abi.section("Trajectory-aligned descriptors of dense tracks", "int ofdis_track_descriptors")
    for words in ("Known value:", "Translation:", "Contract independence:", "Not provided:", "relies on no memset",
                  "ofdis_motion_compensate", r"N\*N\*lmax <= 65536", r"quant\(m, 16\)", r"quant\(m, 256\)", r"quant\(m, 4096\)",
                  r"t = j\*nt / lmax", "does not synchronise with the host"):
        assert re.search(words, section), words


# ------------------------------------------------------------------ the descriptor's size
def _accepted(patch, nxy, nt):
    return 2 <= patch <= 64 and patch % 2 == 0 and 1 <= nxy <= 4 and patch % nxy == 0 and 1 <= nt <= 8


def test_dims_agree_with_the_layout_over_the_whole_range():
    """every (patch, nxy, nt) in and one step around the ranges: D of the layout, 0 exactly for the rejected ones"""
    seen = [0, 0]
    for patch in range(-2, 68):
        for nxy in range(-1, 7):
            for nt in range(-1, 11):
                got = capi.track_descriptor_dims(patch, nxy, nt)
                if _accepted(patch, nxy, nt):
                    layout = tracking.descriptor_layout(patch, nxy, nt)
                    assert got == layout["dims"] == 33 * nxy * nxy * nt, (patch, nxy, nt, got)
                    assert layout["cells"] == (nt, nxy, nxy)
                    cells = nt * nxy * nxy
                    assert layout["channels"] == {"hog": (0, 8), "hof": (8 * cells, 9), "mbhx": (17 * cells, 8),
                                                  "mbhy": (25 * cells, 8)}
                else:
                    assert got == 0, (patch, nxy, nt, got)
                    with pytest.raises(ValueError):
                        tracking.descriptor_layout(patch, nxy, nt)
                seen[got > 0] += 1
    assert min(seen) > 100, seen


# ------------------------------------------------------------------ argument checks
class _Host:
    """host stand-ins for a 4-pair 16x8 case with 64 slots"""

    def __init__(self, w=16, h=8, npairs=4, noc=3):
        self.frames = np.zeros((npairs + 1, h, w, noc), np.uint8)
        self.flow = np.zeros((npairs, h, w, 2), _f32)
        self.tracks = np.zeros((npairs + 1, 64, 2), _f32)
        self.start, self.len, self.info = np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(2, np.int64)
        self.hist = np.zeros((64, 33 * 16 * 8), np.uint32)
        self.shape = np.zeros((64, npairs, 2), _f32)


def _call(hb, frames=True, fw=True, npairs=4, w=16, h=8, noc=1, tracks=True, start=True, length=True, info=True, lmax=3,
          max_tracks=64, patch=8, nxy=2, nt=2, min_flow=0.4, hist=True, shape=True):
    return capi.lib().ofdis_track_descriptors(_p(hb.frames, frames), _p(hb.flow, fw), npairs, w, h, noc, _p(hb.tracks, tracks),
                                              _p(hb.start, start), _p(hb.len, length), _p(hb.info, info), lmax, max_tracks, patch,
                                              nxy, nt, min_flow, _p(hb.hist, hist), _p(hb.shape, shape), None)


@pytest.mark.parametrize("which", ["frames", "fw", "tracks", "start", "length", "info", "hist"])
def test_rejects_null_pointers(which):
    abi.rejected(_call(_Host(), **{which: False}), {"fw": "flow_fw", "length": "len"}.get(which, which))


@pytest.mark.parametrize("kw,word", [
    (dict(noc=0), "noc"), (dict(noc=2), "noc"), (dict(noc=4), "noc"), (dict(noc=-1), "noc"),
    (dict(w=0), "size"), (dict(h=0), "size"), (dict(w=-16), "size"), (dict(w=1 << 16, h=1 << 16), "size"),
    (dict(npairs=0), "npairs"), (dict(npairs=-1), "npairs"),
    (dict(lmax=0), "lmax"), (dict(lmax=-1), "lmax"), (dict(lmax=5), "lmax"), (dict(npairs=2, lmax=3), "lmax"),
    (dict(max_tracks=0), "max_tracks"), (dict(max_tracks=-1), "max_tracks"), (dict(max_tracks=(1 << 24) + 1), "max_tracks"),
    (dict(patch=0), "patch"), (dict(patch=-8), "patch"), (dict(patch=7), "patch"), (dict(patch=66), "patch"),
    (dict(patch=65, nxy=1), "patch"),
    (dict(nxy=0), "nxy"), (dict(nxy=-1), "nxy"), (dict(nxy=5, patch=10), "nxy"), (dict(nxy=3), "nxy"), (dict(nxy=4, patch=6), "nxy"),
    (dict(nt=0), "nt"), (dict(nt=-1), "nt"), (dict(nt=9), "nt"), (dict(nt=4), "nt"), (dict(nt=2, lmax=1), "nt"),
    (dict(min_flow=-0.5), "min_flow"), (dict(min_flow=-math.inf), "min_flow"), (dict(min_flow=math.inf), "min_flow"),
    (dict(min_flow=math.nan), "min_flow"),
], ids=lambda v: ",".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else "")
def test_rejects(kw, word):
    abi.rejected(_call(_Host(), **kw), word)


def test_rejects_a_tube_whose_sums_could_overflow():
    """N * N * lmax <= 65536: at N 64 that is lmax 16"""
    hb = _Host()
    abi.rejected(_call(hb, patch=64, npairs=17, lmax=17), "65536")
    abi.rejected(_call(hb, patch=2, npairs=16385, lmax=16385), "65536")
    abi.rejected(_call(hb, patch=64, npairs=20, lmax=16, min_flow=-1.0), "min_flow")  # 64 * 64 * 16 passes, the next check fails


def test_the_value_checks_accept_their_closed_ranges():
    """both ends of every range: the call passes that check and fails at the last one (min_flow), and with the checks in their
    stated order an earlier failure would name another argument"""
    hb = _Host()
    for kw in (dict(noc=1), dict(noc=3), dict(npairs=3), dict(npairs=1, lmax=1, nt=1), dict(lmax=1, nt=1), dict(lmax=4),
               dict(max_tracks=1), dict(max_tracks=1 << 24), dict(patch=2, nxy=1), dict(patch=2, nxy=2), dict(patch=64, nxy=1),
               dict(patch=64, nxy=4), dict(patch=12, nxy=3), dict(patch=6, nxy=3), dict(nxy=1), dict(nxy=4), dict(nt=1),
               dict(nt=3), dict(npairs=8, lmax=8, nt=8), dict(patch=64, npairs=16, lmax=16), dict(patch=2, npairs=16384, lmax=16384),
               dict(w=1, h=1), dict(w=1 << 15, h=1 << 15), dict(shape=False)):
        abi.rejected(_call(hb, **dict(kw, min_flow=-1.0)), "min_flow")
    # ... and min_flow's own closed end: 0 passes every check.  The call would launch, so it is only made where it cannot:
    # its accepted values are exercised on the device (tests/test_gpu_descriptors.py)
