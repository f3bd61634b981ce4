"""CPU: the global-motion entry points (include/ofdis.h: ofdis_global_motion_work_bytes, ofdis_global_motion,
ofdis_motion_compensate and the two ofdis_batch_* twins) in the header, the binding and the export list, and their argument
checks that return before any device work.  Host buffers stand in for the device arrays: every call here returns before it
would launch.  The kernels, and the checks that need a context (creating one needs a device): tests/test_gpu_gmotion.py."""
import functools
import math
import re

import pytest

import abi
from camera_cases import BAD_SIZES, Host, host_compensate, host_fit
from of_dis_amd import capi

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
# the host stand-ins and the two calls: tests/camera_cases.py, shared with the other model order
_Host = functools.partial(Host, 6)
_fit, _comp = host_fit, host_compensate


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


@pytest.mark.parametrize("npairs,w,h", BAD_SIZES)
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
