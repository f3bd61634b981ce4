"""CPU: the track-selection entry points (include/ofdis.h: ofdis_track_select_defaults, ofdis_track_select_work_bytes,
ofdis_track_select) in the header, the binding and the export list, the defaults, the work buffer's size and the argument checks
that return before any device work.  Host buffers stand in for the device arrays: every call here returns before it would
launch.  The kernels: tests/test_gpu_track_select.py; the definition: tests/test_track_select_ref.py."""
import math
import os
import re

import numpy as np
import pytest

import abi
from of_dis_amd import capi, tracking

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f32 = np.float32
_p = abi.ptr


def test_the_struct_matches_the_header():
    src = abi.header()
    body = re.search(r"typedef struct ofdis_track_select_params \{(.*?)\} ofdis_track_select_params;", src, re.S).group(1)
    fields = re.findall(r"^\s*(int|float|unsigned)\s+(\w+);", body, re.M)
    ctype = {"int": capi.C.c_int, "float": capi.C.c_float, "unsigned": capi.C.c_uint}
    assert [(n, ctype[t]) for t, n in fields] == capi.TrackSelectParams._fields_
    assert capi.C.sizeof(capi.TrackSelectParams) == 28


def test_the_lanes_match_the_kernel_source():
    assert f"kTsLanes = {capi.TRACK_SELECT_LANES};" in open(os.path.join(ROOT, "of_dis_amd", "csrc", "ofdis_track_select.hip")).read()


def test_the_defaults():
    p = capi.TrackSelectParams()
    assert p.min_len == 0 and p.tests == 0x3F
    as32 = lambda v: _f32(v).view(np.uint32)
    assert as32(p.min_std) == as32(1.7320508) == as32(np.sqrt(_f32(3.0)))
    assert (p.max_std, p.max_step, p.min_camera) == (50.0, 20.0, 1.0) and as32(p.max_step_share) == as32(0.7)
    q = tracking.TrackSelectParams()
    for name, _ in capi.TrackSelectParams._fields_:
        assert getattr(p, name) == getattr(q, name), name
    # the call overwrites whatever the struct held, and ignores NULL
    raw = (capi.C.c_ubyte * 28)(*([0xAB] * 28))
    capi.lib().ofdis_track_select_defaults(raw)
    assert bytes(raw) == bytes(p)
    capi.lib().ofdis_track_select_defaults(None)
    assert capi.TrackSelectParams(min_len=3, tests=5).min_len == 3 and capi.TrackSelectParams.of(q).max_std == 50.0


def test_the_header_states_the_definition_and_its_consequences():
    hdr = abi.header()
    section = abi.section("Track selection: the stage", "int ofdis_track_select(")
    for words in ("Drop-in:", "Identity:", "Sums:", "Known values:", "Contract independence:", "Not provided:", "relies on no memset",
                  "FIRST test that holds", "sequential over ascending j", r"L < max\(min_len, 1\)", r"sx < min_std && sy < min_std",
                  r"sx > max_std \|\| sy > max_std", r"mmax > max_step && mmax > S \* max_step_share", r"rmax <= min_camera",
                  r"mu = \(af0 \+ af1\*xc\) \+ af2\*yc", "bit-identical to what ofdis_track_descriptors writes",
                  r"outputs must not\s+\*?\s*overlap", "track_select_ref", "ofdis_batch_global_motion", "nothing synchronises"):
        assert re.search(words, section), words
    # the two sections that used to list the selection as missing
    for name in ("int ofdis_track_descriptors", "int ofdis_track_bof"):
        before = hdr[:hdr.index(name)]
        assert "filtering of static" not in before[before.rindex("Not provided:"):]


# ------------------------------------------------------------------ the work buffer
def test_work_bytes():
    wb = capi.track_select_work_bytes
    lanes = capi.TRACK_SELECT_LANES
    for bad in (0, -1, -(1 << 31), (1 << 24) + 1, (1 << 31) - 1):
        assert wb(bad) == 0, bad
    sizes = [1, 2, lanes - 1, lanes, lanes + 1, 1000, lanes * lanes, lanes * lanes + 1, 1 << 20, (1 << 24) - 1, 1 << 24]
    got = [wb(n) for n in sizes]
    assert all(g > 0 and g % 8 == 0 for g in got), got
    assert got == sorted(got)
    # one 64-byte record per workgroup of TRACK_SELECT_LANES slots: this ties the constant the GPU test sizes its second scan
    # trip by to the library
    assert got == [64 * -(-n // lanes) for n in sizes]
    assert wb(1 << 24) == 64 * 65536 < 1 << 23


# ------------------------------------------------------------------ argument checks
class _Host:
    """host stand-ins for 64 slots of lmax 3, 5 pairs of models"""

    def __init__(self):
        self.tracks, self.tracks_out = np.zeros((4, 64, 2), _f32), np.zeros((4, 64, 2), _f32)
        self.start, self.len, self.info = np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(2, np.int64)
        self.start_out, self.len_out, self.info_out = np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(2, np.int64)
        self.models = np.zeros((5, 6), np.float64)
        self.code, self.counts, self.index = np.zeros(64, np.uint8), np.zeros(7, np.int64), np.zeros(64, np.int32)
        self.shape = np.zeros((64, 3, 2), _f32)
        self.work = np.zeros(64, np.uint64)


def _call(hb, tracks=True, start=True, length=True, info=True, lmax=3, max_tracks=64, models=False, npairs=5, w=16, h=8, params=True,
          code=True, counts=True, max_tracks_out=64, tracks_out=True, start_out=True, len_out=True, info_out=True, index=True,
          shape=True, work=True, work_bytes=None, work_offset=0, **fields):
    p = capi.TrackSelectParams(**fields)
    need = capi.track_select_work_bytes(max_tracks)
    return capi.lib().ofdis_track_select(
        _p(hb.tracks, tracks), _p(hb.start, start), _p(hb.len, length), _p(hb.info, info), lmax, max_tracks, _p(hb.models, models),
        npairs, w, h, capi.C.byref(p) if params else None, _p(hb.code, code), _p(hb.counts, counts), max_tracks_out,
        _p(hb.tracks_out, tracks_out), _p(hb.start_out, start_out), _p(hb.len_out, len_out), _p(hb.info_out, info_out),
        _p(hb.index, index), _p(hb.shape, shape), _p(hb.work, work) + work_offset if work else None,
        need if work_bytes is None else work_bytes, None)


@pytest.mark.parametrize("which", ["tracks", "start", "length", "info", "params", "tracks_out", "start_out", "len_out", "info_out", "work"])
def test_rejects_null_pointers(which):
    abi.rejected(_call(_Host(), **{which: False}), {"length": "len"}.get(which, which))


@pytest.mark.parametrize("kw,word", [
    (dict(lmax=0), "lmax"), (dict(lmax=-3), "lmax"),
    (dict(max_tracks=0), "max_tracks"), (dict(max_tracks=-1), "max_tracks"), (dict(max_tracks=(1 << 24) + 1), "max_tracks"),
    (dict(max_tracks_out=0), "max_tracks_out"), (dict(max_tracks_out=-1), "max_tracks_out"),
    (dict(max_tracks_out=(1 << 24) + 1), "max_tracks_out"),
    (dict(models=True, npairs=0), "models"), (dict(models=True, npairs=-1), "models"), (dict(models=True, w=0), "models"),
    (dict(models=True, h=0), "models"), (dict(models=True, h=-8), "models"), (dict(models=True, w=8193), "models"),
    (dict(models=True, h=8193), "models"),
    (dict(min_len=-1), "min_len"),
    (dict(min_std=-0.5), "min_std"), (dict(min_std=math.nan), "min_std"), (dict(min_std=math.inf), "min_std"),
    (dict(max_std=-1.0), "max_std"), (dict(max_std=math.nan), "max_std"), (dict(max_std=-math.inf), "max_std"),
    (dict(max_step=-1.0), "max_step"), (dict(max_step=math.nan), "max_step"), (dict(max_step=-math.inf), "max_step"),
    (dict(max_step_share=-0.1), "max_step_share"), (dict(max_step_share=1.5), "max_step_share"),
    (dict(max_step_share=math.nan), "max_step_share"), (dict(max_step_share=math.inf), "max_step_share"),
    (dict(min_camera=-1.0), "min_camera"), (dict(min_camera=math.nan), "min_camera"), (dict(min_camera=math.inf), "min_camera"),
    (dict(tests=0x40), "tests"), (dict(tests=0x7F), "tests"), (dict(tests=1 << 31), "tests"),
    (dict(work_bytes=0), "work"), (dict(work_bytes=63), "work"), (dict(max_tracks=257, work_bytes=64), "work"),
    (dict(work_offset=4), "work"), (dict(work_offset=1), "work"),
], ids=lambda v: ",".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else "")
def test_rejects(kw, word):
    abi.rejected(_call(_Host(), **kw), word)


def test_the_value_checks_accept_their_closed_ranges():
    """both ends of every range and every optional pointer left out: the call passes that check and fails at the last one (the
    work buffer), and with the checks in their stated order an earlier failure would name another argument"""
    hb = _Host()
    for kw in (dict(lmax=1), dict(lmax=1 << 20), dict(max_tracks=1), dict(max_tracks=1 << 24), dict(max_tracks_out=1),
               dict(max_tracks_out=1 << 24), dict(models=True, npairs=1, w=1, h=1), dict(models=True, w=8192, h=8192),
               dict(models=False, npairs=0, w=0, h=0), dict(models=False, npairs=-1, w=1 << 20, h=-5),
               dict(min_len=0), dict(min_len=1 << 20), dict(min_std=0.0), dict(max_std=0.0), dict(max_std=math.inf),
               dict(max_step=0.0), dict(max_step=math.inf), dict(max_step_share=0.0), dict(max_step_share=1.0),
               dict(min_camera=0.0), dict(tests=0), dict(tests=0x3F), dict(tests=0x20),
               dict(code=False), dict(counts=False), dict(index=False), dict(shape=False),
               dict(code=False, counts=False, index=False, shape=False)):
        abi.rejected(_call(hb, **dict(kw, work_bytes=8)), "work")
    # ... and the work buffer's own closed end, ofdis_track_select_work_bytes exactly, passes every check.  The call would
    # launch, so it is only made where it cannot: its accepted values are exercised on the device (tests/test_gpu_track_select.py)
