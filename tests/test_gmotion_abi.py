"""CPU: the global-motion entry points (include/ofdis.h: ofdis_global_motion_work_bytes, ofdis_global_motion,
ofdis_motion_compensate and the two ofdis_batch_* twins) in the header, the binding and the export list, and their argument
checks that return before any device work.  Host buffers stand in for the device arrays: every call here returns before it
would launch.  The kernels, and the checks that need a context (creating one needs a device): tests/test_gpu_gmotion.py."""
import math
import re

import numpy as np
import pytest

import abi
from of_dis_amd import capi

_f32 = np.float32
_p = abi.ptr


def test_the_header_derives_the_bound_and_names_the_caveat():
    section = re.sub(r"\s+\*?\s*", " ", abi.section("Global (camera) motion models", "#define OFDIS_GM_MAX_SIDE"))
    assert "2^59" in section and "int64 never overflows" in section
    assert "det == 0 exactly" in section and "only approximately 0" in section
    for word in ("homography", "similarity", "stabilisation", "reverse direction", "sequence driver"):
        assert word in section, word


# ------------------------------------------------------------------ ofdis_global_motion_work_bytes
def test_work_bytes():
    wb = capi.lib().ofdis_global_motion_work_bytes
    assert wb(1, 1, 1) == 96                                 # one workgroup, one record
    assert wb(1, 256, 112) == 96 * ((64 * 112 + 255) // 256)
    sizes = [wb(n, 300, 70) for n in (1, 2, 3, 10, 1000)]
    assert all(s > 0 for s in sizes) and sizes == sorted(set(sizes)) and sizes[3] == 10 * sizes[0]
    assert wb(1, 8192, 8192) == 96 * (2048 * 8192 // 256)
    for bad in ((0, 8, 4), (-1, 8, 4), (1, 0, 4), (1, 8, 0), (1, -8, 4), (1, 8193, 4), (1, 4, 8193), (1, 1 << 16, 1 << 16)):
        assert wb(*bad) == 0, bad


# ------------------------------------------------------------------ argument checks
class _Host:
    """host stand-ins for a 2-pair 8x4 case"""

    def __init__(self, w=8, h=4, npairs=2):
        self.flow = np.zeros((npairs, h, w, 2), _f32)
        self.mask = np.zeros((npairs, h, w), np.uint8)
        self.models = np.zeros((npairs, 6), np.float64)
        self.stats = np.zeros((npairs, 3), np.int64)
        self.work = np.zeros(4096, np.int64)
        self.residual = np.zeros((npairs, h, w, 2), _f32)
        self.label = np.zeros((npairs, h, w), np.uint8)


def _fit(hb, flow=True, models=True, work=True, work_bytes=None, work_off=0, npairs=2, w=8, h=4, model=1, rounds=3, thresh=1.0):
    wb = hb.work.nbytes - 8 if work_bytes is None else work_bytes
    wp = hb.work.ctypes.data + work_off if work else None
    return capi.lib().ofdis_global_motion(_p(hb.flow, flow), _p(hb.mask), npairs, w, h, model, rounds, thresh,
                                          _p(hb.models, models), _p(hb.stats), wp, wb, None)


def _comp(hb, flow=True, models=True, residual=True, label=True, npairs=2, w=8, h=4, thresh=1.0):
    return capi.lib().ofdis_motion_compensate(_p(hb.flow, flow), _p(hb.mask), _p(hb.models, models), npairs, w, h, thresh,
                                              _p(hb.residual, residual), _p(hb.label, label), None)


@pytest.mark.parametrize("which", ["flow", "models"])
def test_null_pointers(which):
    abi.rejected(_fit(_Host(), **{which: False}))
    abi.rejected(_comp(_Host(), **{which: False}))


def test_compensate_needs_an_output():
    abi.rejected(_comp(_Host(), residual=False, label=False))


@pytest.mark.parametrize("model", [-1, 2, 3, 1 << 20])
def test_rejects_model(model):
    abi.rejected(_fit(_Host(), model=model), "model")


@pytest.mark.parametrize("rounds", [0, -1, 9, 1 << 20])
def test_rejects_rounds(rounds):
    abi.rejected(_fit(_Host(), rounds=rounds), "rounds")


@pytest.mark.parametrize("thresh", [0.0, -0.0, -1.0, math.nan, math.inf, -math.inf])
def test_rejects_thresh(thresh):
    abi.rejected(_fit(_Host(), thresh=thresh), "thresh")
    abi.rejected(_comp(_Host(), thresh=thresh), "thresh")


SIZES = [(0, 8, 4), (-1, 8, 4), (2, 0, 4), (2, 8, 0), (2, -8, 4), (2, 1 << 16, 1 << 16), (2, 8193, 4), (2, 8, 8193)]


@pytest.mark.parametrize("npairs,w,h", SIZES)
def test_rejects_bad_sizes(npairs, w, h):
    abi.rejected(_fit(_Host(), npairs=npairs, w=w, h=h), "size")
    abi.rejected(_comp(_Host(), npairs=npairs, w=w, h=h), "size")


def test_rejects_the_work_buffer():
    need = capi.lib().ofdis_global_motion_work_bytes(2, 8, 4)
    assert need == 2 * 96
    abi.rejected(_fit(_Host(), work=False), "work")
    abi.rejected(_fit(_Host(), work_bytes=need - 1), "work")
    abi.rejected(_fit(_Host(), work_bytes=0), "work")
    abi.rejected(_fit(_Host(), work_off=4), "work")


def test_the_value_checks_accept_their_ranges():
    """both models, rounds 1 and 8, tiny and huge thresholds, the largest side: the call gets as far as the work-buffer check"""
    for kw in (dict(model=0), dict(model=1), dict(rounds=1), dict(rounds=8), dict(thresh=1e-30), dict(thresh=3e38),
               dict(w=8192, h=1), dict(w=1, h=8192)):
        abi.rejected(_fit(_Host(), work=False, **kw), "work")


def test_batch_calls_without_a_context():
    hb = _Host()
    L = capi.lib()
    abi.rejected(L.ofdis_batch_global_motion(None, 0, 2, 1, 3, 1.0, 0, capi.FB_ALPHA, capi.FB_BETA, _p(hb.models), _p(hb.stats), 8, 4,
                                          None))
    abi.rejected(L.ofdis_batch_motion_compensate(None, 0, 2, _p(hb.models), 1.0, 0, capi.FB_ALPHA, capi.FB_BETA, _p(hb.residual),
                                              _p(hb.label), 8, 4, None))
