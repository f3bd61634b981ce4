"""CPU: the object-track entry points (include/ofdis.h: ofdis_segment_tracks_work_bytes, ofdis_segment_overlap, _link, _chain,
_relabel, _tracks) in the header and the binding, and their argument checks that return before any device work.  Host buffers
stand in for the device arrays: every call here returns before it would launch.  The kernels: tests/test_gpu_segment_tracks.py."""
import ctypes as C
import re

import numpy as np
import pytest

import abi
from of_dis_amd import capi, segments as S

_p = abi.ptr
BAD_SIZES = [(2, 0, 4), (2, 8, 0), (2, -8, 4), (2, 1 << 16, 1 << 16), (2, 8193, 4), (2, 8, 8193)]
BAD_NMAPS = [0, -1, 65537, (1 << 31) - 1]
BAD_SEGMENTS = [0, -1, 1025, 1 << 24]
BAD_SHARE = [-1, 101, 1 << 20]
BAD_TRACKS = [0, -1, (1 << 24) + 1, (1 << 31) - 1]


class Host:
    """host stand-ins for a 2-map 8x4 case with 4 segment slots and 8 track slots"""

    def __init__(self):
        self.segments = np.zeros((2, 4, 8), np.int32)
        self.flow = np.zeros((2, 4, 8, 2), np.float32)
        self.records = np.zeros((2, 4, 12), np.int64)
        self.info = np.zeros((2, 4), np.int64)
        self.overlap = np.zeros((1, 4, 4), np.int32)
        self.link = np.zeros((1, 4), np.int32)
        self.ids = np.zeros((2, 4), np.int32)
        self.tracks = np.zeros((8, 12), np.int64)
        self.tinfo = np.zeros(4, np.int64)
        self.track_map = np.zeros((2, 4, 8), np.int32)
        self.work = np.zeros(4096, np.int64)


# the calls: name -> (pointer arguments in order, which of the value arguments it takes)
def _overlap(hb, off=(), nmaps=2, w=8, h=4, S_=4, **_):
    q = lambda n: _p(getattr(hb, n), n not in off)
    return capi.lib().ofdis_segment_overlap(q("segments"), q("flow"), q("info"), nmaps, w, h, S_, q("overlap"), None)


def _link(hb, off=(), nmaps=2, S_=4, min_share=50, **_):
    q = lambda n: _p(getattr(hb, n), n not in off)
    return capi.lib().ofdis_segment_link(q("overlap"), q("records"), q("info"), nmaps, S_, min_share, q("link"), None)


def _chain(hb, off=(), nmaps=2, S_=4, max_tracks=8, **_):
    q = lambda n: _p(getattr(hb, n), n not in off)
    return capi.lib().ofdis_segment_chain(q("link"), q("records"), q("info"), nmaps, S_, max_tracks, q("ids"), q("tracks"), q("tinfo"),
                                          None)


def _relabel(hb, off=(), nmaps=2, w=8, h=4, S_=4, **_):
    q = lambda n: _p(getattr(hb, n), n not in off)
    return capi.lib().ofdis_segment_relabel(q("segments"), q("ids"), q("info"), nmaps, w, h, S_, q("track_map"), None)


def _tracks(hb, off=(), nmaps=2, w=8, h=4, S_=4, min_share=50, max_tracks=8, work=True, work_bytes=None, work_off=0):
    q = lambda n: _p(getattr(hb, n), n not in off)
    wb = hb.work.nbytes - 8 if work_bytes is None else work_bytes
    wp = hb.work.ctypes.data + work_off if work else None
    return capi.lib().ofdis_segment_tracks(q("segments"), q("flow"), q("records"), q("info"), nmaps, w, h, S_, min_share, max_tracks,
                                           q("ids"), q("tracks"), q("tinfo"), q("track_map"), wp, wb, None)


REQUIRED = {_overlap: ("segments", "flow", "info", "overlap"), _link: ("overlap", "records", "info", "link"),
            _chain: ("link", "records", "info", "ids", "tracks", "tinfo"), _relabel: ("segments", "ids", "info", "track_map"),
            _tracks: ("segments", "flow", "records", "info", "ids", "tracks", "tinfo")}
WITH_FRAME, WITH_SHARE, WITH_TRACKS = (_overlap, _relabel, _tracks), (_link, _tracks), (_chain, _tracks)
CALLS = list(REQUIRED)
_ids = lambda f: f.__name__


def _flat(text):
    """a comment's text on one line: line breaks with their leading ` * ` folded into one blank (a ` * ` inside a line goes too)"""
    return re.sub(r"\s+\*?\s*", " ", text)


def test_the_header_derives_the_bounds_and_lists_what_is_not_provided():
    section = _flat(abi.section("Object tracks: the segments of consecutive maps", "size_t ofdis_segment_tracks_work_bytes"))
    assert "Not provided:" in section
    for word in ("split and merge events", "across a gap", "sparse overlap for more than 1024 segments", "level flows directly",
                 "sequence driver"):
        assert word in section, word
    for word in ("N*S <= 2^26 fits int32", "2^39 * 2^16", "2^46 * 2^16 = 2^62", "int64 never overflows", "W*H < 2^26",
                 "associative and commutative", "pure function of the inputs"):
        assert _flat(word) in section, word
    for word in ("min(max(info[k][2], 0), S)", "1 <= s <= n_k", "(int)rintf(u)", "fabsf(u) <= 4096", "a NaN fails", "among equals the smallest b",
                 "c * 100 >= min_share * min(area_k(a), area_{k+1}(b))", "clamped to 0 .. 2^26", "injective", "ordered by k, then by s",
                 "two's-complement", "neither read nor written", "every entry is written once", "S <= 128", "adds no macro",
                 "1 .. 65536", "1 .. 1024", "0 .. 100", "1 .. 16777216", "SEGTRACK_MAX_SEGMENTS = 1024", "SEGTRACK_MAX_MAPS = 65536",
                 "SEGTRACK_MAX_TRACKS = 2^24", "SEGTRACK_FIELDS = 12", "SEGTRACK_INFO_FIELDS = 4", "SEGTRACK_LDS_MAX_SEGMENTS = 128",
                 "no floating-point atomic", "no workgroup waits for another"):
        assert _flat(word) in section, word
    segments = _flat(abi.section("Segments: connected components of a label map", "size_t ofdis_segments_work_bytes"))
    assert "Object tracks" in segments and "ofdis_segment_tracks" in segments   # the pointer from the section before


def test_the_limits_are_mirrored():
    for mod in (capi, S):
        assert (mod.SEGTRACK_MAX_SEGMENTS, mod.SEGTRACK_MAX_MAPS, mod.SEGTRACK_MAX_TRACKS) == (1024, 65536, 1 << 24)
        assert (mod.SEGTRACK_FIELDS, mod.SEGTRACK_INFO_FIELDS, mod.SEGTRACK_LDS_MAX_SEGMENTS) == (12, 4, 128)
    assert capi.SEGTRACK_LDS_MAX_SEGMENTS ** 2 * 4 == 64 * 1024
    # the grid caps and the band: the kernels' constants (the file states each once)
    src = open(capi._HERE + "/csrc/ofdis_segment_tracks.hip").read()
    consts = dict(re.findall(r"constexpr int (kSt\w+) = ([^;]+);", src))
    assert eval(consts["kStGridBlocks"], {}, {k: int(v) for k, v in consts.items() if v.isdigit()}) == capi.SEGTRACK_GRID_BLOCKS == 2048
    assert eval(consts["kStLdsGridBlocks"], {}, {k: int(v) for k, v in consts.items() if v.isdigit()}) == capi.SEGTRACK_LDS_GRID_BLOCKS == 512
    assert int(consts["kStBandRows"]) == capi.SEGTRACK_BAND_ROWS and int(consts["kStLdsMaxSegments"]) == capi.SEGTRACK_LDS_MAX_SEGMENTS
    assert int(consts["kStMaxSegments"]) == capi.SEGTRACK_MAX_SEGMENTS and int(consts["kStRecord"]) == capi.SEGTRACK_FIELDS


def test_the_six_functions_are_declared_with_the_closed_type_set():
    V, I, Z = C.c_void_p, C.c_int, C.c_size_t
    protos = capi._prototypes()
    assert protos["ofdis_segment_tracks_work_bytes"] == (Z, [I, I])
    assert protos["ofdis_segment_overlap"] == (I, [V, V, V, I, I, I, I, V, V])
    assert protos["ofdis_segment_link"] == (I, [V, V, V, I, I, I, V, V])
    assert protos["ofdis_segment_chain"] == (I, [V, V, V, I, I, I, V, V, V, V])
    assert protos["ofdis_segment_relabel"] == (I, [V, V, V, I, I, I, I, V, V])
    assert protos["ofdis_segment_tracks"] == (I, [V, V, V, V, I, I, I, I, I, I, V, V, V, V, V, Z, V])
    names = list(protos)
    at = names.index("ofdis_label_segments")   # the section stands right after "Segments"
    assert names[at + 1:at + 7] == ["ofdis_segment_tracks_work_bytes", "ofdis_segment_overlap", "ofdis_segment_link",
                                    "ofdis_segment_chain", "ofdis_segment_relabel", "ofdis_segment_tracks"]


# ------------------------------------------------------------------ ofdis_segment_tracks_work_bytes
def test_work_bytes():
    wb = capi.lib().ofdis_segment_tracks_work_bytes
    for nmaps, s in ((1, 1), (1, 1024), (2, 1), (2, 2), (3, 3), (4, 5), (7, 128), (7, 129), (1025, 256), (65536, 1024)):
        want = max(8, -(-((nmaps - 1) * s * (s + 1) * 4) // 8) * 8)
        assert wb(nmaps, s) == want == S.segment_tracks_work_bytes(nmaps, s) == capi.segment_tracks_work_bytes(nmaps, s), (nmaps, s)
    assert wb(1, 1) == 8 and wb(2, 2) == 24 and wb(4, 5) == 360 and wb(65536, 1024) == 65535 * 1024 * 1025 * 4
    for bad in [(n, 4) for n in BAD_NMAPS] + [(2, s) for s in BAD_SEGMENTS]:
        assert wb(*bad) == 0 == S.segment_tracks_work_bytes(*bad), bad


# ------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("call,which", [(f, w) for f in CALLS for w in REQUIRED[f]], ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_null_pointers(call, which):
    abi.rejected(call(Host(), off=(which,)), which)


@pytest.mark.parametrize("call", CALLS, ids=_ids)
@pytest.mark.parametrize("nmaps", BAD_NMAPS)
def test_rejects_nmaps(call, nmaps):
    abi.rejected(call(Host(), nmaps=nmaps), "nmaps")


@pytest.mark.parametrize("call", CALLS, ids=_ids)
@pytest.mark.parametrize("s", BAD_SEGMENTS)
def test_rejects_max_segments(call, s):
    abi.rejected(call(Host(), S_=s), "max_segments")


@pytest.mark.parametrize("call", WITH_SHARE, ids=_ids)
@pytest.mark.parametrize("min_share", BAD_SHARE)
def test_rejects_min_share(call, min_share):
    abi.rejected(call(Host(), min_share=min_share), "min_share")


@pytest.mark.parametrize("call", WITH_TRACKS, ids=_ids)
@pytest.mark.parametrize("max_tracks", BAD_TRACKS)
def test_rejects_max_tracks(call, max_tracks):
    abi.rejected(call(Host(), max_tracks=max_tracks), "max_tracks")


@pytest.mark.parametrize("call", WITH_FRAME, ids=_ids)
@pytest.mark.parametrize("nmaps,w,h", BAD_SIZES)
def test_rejects_bad_sizes(call, nmaps, w, h):
    abi.rejected(call(Host(), nmaps=nmaps, w=w, h=h), "size")


def test_rejects_the_work_buffer():
    need = capi.lib().ofdis_segment_tracks_work_bytes(2, 4)
    assert need == 4 * 5 * 4
    abi.rejected(_tracks(Host(), work=False), "work")
    abi.rejected(_tracks(Host(), work_bytes=need - 1), "work")
    abi.rejected(_tracks(Host(), work_bytes=0), "work")
    abi.rejected(_tracks(Host(), work_off=4), "work")


def test_the_value_checks_accept_their_ranges():
    """the extremes of every range, the largest sides and no track_map: the composite gets as far as the work-buffer check"""
    for kw in (dict(nmaps=1), dict(nmaps=65536), dict(S_=1), dict(S_=1024), dict(min_share=0), dict(min_share=100),
               dict(max_tracks=1), dict(max_tracks=1 << 24), dict(w=8192, h=1), dict(w=1, h=8192), dict(off=("track_map",))):
        abi.rejected(_tracks(Host(), work=False, **kw), "work")
