"""The launch hook of the segment labelling (tests/csrc/ofdis_launch_hooks_segments.hip): launch_label_segments of the TEST
library, whose GRID_MAX_BLOCKS a test lowers through launch_hooks.launch_limits so that every one of its grid-stride kernels
makes a second trip at test sizes.  libofdis_hip.so is a separate object: nothing here changes what it does."""
import ctypes as C

import numpy as np

import launch_hooks
from of_dis_amd import segments as S

_I, _VP = C.c_int, C.c_void_p


def _hooks():
    L = launch_hooks.hooks()
    L.ofdis_test_launch_label_segments.argtypes = [_VP, _VP, _I, _I, _I, C.c_uint, _I, _I, _I, _VP, _VP, _VP, _VP, _VP]
    L.ofdis_test_launch_label_segments.restype = _I
    L.ofdis_test_segments_work_bytes.argtypes, L.ofdis_test_segments_work_bytes.restype = [_I, _I, _I], C.c_size_t
    return L


def work_bytes(nmaps, w, h):
    return int(_hooks().ofdis_test_segments_work_bytes(nmaps, w, h))


def label_segments(gpu, label, flow, codes, conn, min_area, max_segments, records_fill):
    """launch_label_segments of the test library on the null stream -> (segments, records, info) as capi.label_segments"""
    L = _hooks()
    nmaps, h, w = label.shape
    dl = gpu.Dev(label)
    df = gpu.Dev(np.ascontiguousarray(flow, np.float32)) if flow is not None else None
    ds, dr = gpu.Dev(nbytes=nmaps * h * w * 4), gpu.Dev(np.ascontiguousarray(records_fill, np.int64))
    di, dw = gpu.Dev(nbytes=nmaps * 32), gpu.Dev(nbytes=work_bytes(nmaps, w, h))
    rc = L.ofdis_test_launch_label_segments(dl.ptr, df.ptr if df else None, nmaps, w, h, codes, conn, min_area, max_segments, ds.ptr,
                                            dr.ptr, di.ptr, dw.ptr, None)
    assert rc == 0, f"ofdis_test_launch_label_segments: hipError_t {rc}"
    gpu.check(gpu.lib().ofdis_sync(None))
    return (ds.get((nmaps, h, w), np.int32), dr.get((nmaps, max_segments, S.SEG_RECORD_FIELDS), np.int64),
            di.get((nmaps, S.SEG_INFO_FIELDS), np.int64))
