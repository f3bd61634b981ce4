"""CPU: argument checks of the bidirectional-flow entry points that return before any device work (include/ofdis.h:
ofdis_batch_create_ex, ofdis_fb_check, the reverse getters).  The computations themselves: tests/test_gpu_bidir.py."""
import ctypes as C
import math

import numpy as np
import pytest

import abi
from of_dis_amd import capi
from of_dis_amd.params import oppoint


def test_constants_match_the_header():
    assert abi.define("OFDIS_BATCH_REVERSE") == capi.BATCH_REVERSE
    assert (abi.define("OFDIS_FB_ALPHA"), abi.define("OFDIS_FB_BETA")) == (capi.FB_ALPHA, capi.FB_BETA)
    assert [abi.enumerator("OFDIS_FB_" + n) for n in ("CONSISTENT", "INCONSISTENT", "OUTSIDE")] \
        == [capi.FB_CONSISTENT, capi.FB_INCONSISTENT, capi.FB_OUTSIDE]


def test_create_ex_rejects_stereo_reverse_and_unknown_flags():
    L = capi.lib()
    p = oppoint(2, 256, 112)
    h = C.c_void_p()
    assert L.ofdis_batch_create_ex(C.byref(h), C.byref(p.copy(selectmode=2)), 2, capi.BATCH_REVERSE) == -2  # UNSUPPORTED
    assert not h.value
    for flags in (2, 4, 0x80000000, 0x80000001):
        assert L.ofdis_batch_create_ex(C.byref(h), C.byref(p), 2, flags) == -1  # INVALID
        assert not h.value
    assert L.ofdis_batch_create_ex(C.byref(h), C.byref(p.copy(width=1001)), 2, capi.BATCH_REVERSE) == -1  # bad params first


def test_reverse_getters_without_a_context():
    L = capi.lib()
    assert not L.ofdis_batch_flow_reverse(None)
    assert not L.ofdis_batch_level_flow_reverse(None, 0)
    assert L.ofdis_batch_set_initflow_reverse(None, None) == -1
    assert L.ofdis_batch_download_reverse(None, 0, None, None) == -1
    assert L.ofdis_batch_upsample_bidir(None, 0, 1, None, None, None, None, 16, 16, 0.01, 0.5, None) == -1


@pytest.mark.parametrize("alpha,beta", [(-0.01, 0.5), (0.01, -0.5), (math.inf, 0.5), (0.01, math.inf), (math.nan, 0.5),
                                        (0.01, math.nan), (-0.0 - 1e-30, 0.0)])
def test_fb_check_rejects_bad_constants(alpha, beta):
    """(host buffers stand in for the device arrays: the call returns before it would launch)"""
    L = capi.lib()
    f = np.zeros((1, 4, 4, 2), np.float32)
    m = np.zeros((1, 4, 4), np.uint8)
    assert L.ofdis_fb_check(f.ctypes.data, f.ctypes.data, m.ctypes.data, 1, 4, 4, alpha, beta, None) == -1
    assert "alpha" in L.ofdis_last_error().decode()


@pytest.mark.parametrize("n,w,h", [(0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 1 << 16, 1 << 16)])
def test_fb_check_rejects_bad_sizes(n, w, h):
    L = capi.lib()
    f = np.zeros(8, np.float32)
    assert L.ofdis_fb_check(f.ctypes.data, f.ctypes.data, f.ctypes.data, n, w, h, 0.01, 0.5, None) == -1
    assert L.ofdis_fb_check(None, f.ctypes.data, f.ctypes.data, 1, 1, 1, 0.01, 0.5, None) == -1
