"""CPU: the segment entry points (include/ofdis.h: ofdis_segments_work_bytes, ofdis_label_segments) in the header and the
binding, and their argument checks that return before any device work.  Host buffers stand in for the device arrays: every
call here returns before it would launch.  The kernels: tests/test_gpu_segments.py."""
import re

import numpy as np
import pytest

import abi
from of_dis_amd import capi, segments as S

_p = abi.ptr
BAD_SIZES = [(0, 8, 4), (-1, 8, 4), (2, 0, 4), (2, 8, 0), (2, -8, 4), (2, 1 << 16, 1 << 16), (2, 8193, 4), (2, 8, 8193)]


class Host:
    """host stand-ins for a 2-map 8x4 case"""

    def __init__(self):
        self.label = np.zeros((2, 4, 8), np.uint8)
        self.flow = np.zeros((2, 4, 8, 2), np.float32)
        self.segments = np.zeros((2, 4, 8), np.int32)
        self.records = np.zeros((2, 4, 12), np.int64)
        self.info = np.zeros((2, 4), np.int64)
        self.work = np.zeros(4096, np.int64)


def _call(hb, label=True, flow=True, segments=True, records=True, info=True, work=True, work_bytes=None, work_off=0, nmaps=2, w=8,
          h=4, codes=2, conn=8, min_area=0, max_segments=4):
    wb = hb.work.nbytes - 8 if work_bytes is None else work_bytes
    wp = hb.work.ctypes.data + work_off if work else None
    return capi.lib().ofdis_label_segments(_p(hb.label, label), _p(hb.flow, flow), nmaps, w, h, codes, conn, min_area, max_segments,
                                           _p(hb.segments, segments), _p(hb.records, records), _p(hb.info, info), wp, wb, None)


def test_the_header_derives_the_bounds_and_lists_what_is_not_provided():
    section = re.sub(r"\s+\*?\s*", " ", abi.section("Segments: connected components of a label map", "size_t ofdis_segments_work_bytes"))
    assert "below 2^26 and fits int32" in section and "2^39" in section and "2^46" in section and "int64 never overflows" in section
    assert "associative and commutative" in section and "pure function of the inputs" in section
    assert "Not provided:" in section
    for word in ("opening or closing", "hole filling", "across frames", "level flows directly", "sequence driver"):
        assert word in section, word
    for word in ("label[p] < 8", "max(min_area, 1)", "scipy.ndimage.label", "min(nkept, max_segments)", "(int)rintf(u",
                 "neither read nor written", "1 .. 16777216", "adds no macro"):
        assert word in section, word


def test_the_two_functions_are_declared_with_the_closed_type_set():
    import ctypes as C
    V, I = C.c_void_p, C.c_int
    protos = capi._prototypes()
    assert protos["ofdis_segments_work_bytes"] == (C.c_size_t, [I, I, I])
    assert protos["ofdis_label_segments"] == (I, [V, V, I, I, I, C.c_uint, I, I, I, V, V, V, V, C.c_size_t, V])


# ------------------------------------------------------------------ ofdis_segments_work_bytes
def test_work_bytes():
    wb = capi.lib().ofdis_segments_work_bytes
    for nmaps, w, h in ((1, 1, 1), (1, 64, 16), (3, 64, 16), (1, 8192, 8192), (2, 300, 70)):
        n = w * h
        assert wb(nmaps, w, h) == nmaps * (8 * n + 16 * ((n + 255) // 256)) == S.segments_work_bytes(nmaps, w, h), (nmaps, w, h)
    assert wb(1, 1, 1) == 24 and wb(1, 64, 16) == 8 * 1024 + 64 and wb(1, 8192, 8192) == (8 << 26) + (16 << 18)
    sizes = [wb(n, 300, 70) for n in (1, 2, 3, 10, 1000)]
    assert all(s > 0 for s in sizes) and sizes == sorted(set(sizes)) and sizes[3] == 10 * sizes[0]
    for bad in BAD_SIZES + [(1, 8193, 1), (1, 1, 8193)]:
        assert wb(*bad) == 0 == S.segments_work_bytes(*bad), bad


# ------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("which", ["label", "info"])
def test_null_pointers(which):
    abi.rejected(_call(Host(), **{which: False}), which)


def test_needs_an_output():
    abi.rejected(_call(Host(), segments=False, records=False), "segments and records")


@pytest.mark.parametrize("codes", [0, 0x100, 0x1FF, 1 << 31, 0xFFFFFFFF])
def test_rejects_codes(codes):
    abi.rejected(_call(Host(), codes=codes), "codes")


@pytest.mark.parametrize("conn", [0, 1, 6, -8, 16])
def test_rejects_conn(conn):
    abi.rejected(_call(Host(), conn=conn), "conn")


@pytest.mark.parametrize("min_area", [-1, -(1 << 31)])
def test_rejects_min_area(min_area):
    abi.rejected(_call(Host(), min_area=min_area), "min_area")


@pytest.mark.parametrize("max_segments", [0, -1, (1 << 24) + 1, (1 << 31) - 1])
def test_rejects_max_segments(max_segments):
    abi.rejected(_call(Host(), max_segments=max_segments), "max_segments")


@pytest.mark.parametrize("nmaps,w,h", BAD_SIZES)
def test_rejects_bad_sizes(nmaps, w, h):
    abi.rejected(_call(Host(), nmaps=nmaps, w=w, h=h), "size")


def test_rejects_the_work_buffer():
    need = capi.lib().ofdis_segments_work_bytes(2, 8, 4)
    assert need == 2 * (8 * 32 + 16)
    abi.rejected(_call(Host(), work=False), "work")
    abi.rejected(_call(Host(), work_bytes=need - 1), "work")
    abi.rejected(_call(Host(), work_bytes=0), "work")
    abi.rejected(_call(Host(), work_off=4), "work")


def test_the_value_checks_accept_their_ranges():
    """both connectivities, min_area 0, max_segments 1 and 16777216, codes 0xFF, either output alone, no flow, the largest
    sides: the call gets as far as the work-buffer check"""
    for kw in (dict(conn=4), dict(conn=8), dict(min_area=0), dict(min_area=(1 << 31) - 1), dict(max_segments=1),
               dict(max_segments=1 << 24), dict(codes=0xFF), dict(codes=1), dict(segments=False), dict(records=False),
               dict(flow=False), dict(w=8192, h=1), dict(w=1, h=8192)):
        abi.rejected(_call(Host(), work=False, **kw), "work")
