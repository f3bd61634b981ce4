"""CPU: the stereo left-right step (include/ofdis.h: OFDIS_BATCH_STEREO_LR, ofdis_lr_check, ofdis_disparity_fill,
ofdis_batch_upsample_lr).  Argument checks that return before any device work, and the numpy restatement
(tests/stereo_lr_ref.py) on the reference build's disparities of the Middlebury pair: what the check and the fill are worth.
The computations on the device: tests/test_gpu_stereo_lr.py."""
import ctypes as C
import math

import numpy as np
import pytest

import abi
import natural
import oracle
import stereo_lr_ref as ref
from of_dis_amd import capi
from of_dis_amd.params import oppoint

ALPHA, BETA = 0.01, 0.5  # (the issue's constants; OFDIS_FB_ALPHA / OFDIS_FB_BETA)


def test_constants_match_the_header():
    assert abi.define("OFDIS_BATCH_STEREO_LR") == capi.BATCH_STEREO_LR == 2
    fills = tuple(abi.enumerator("OFDIS_FILL_" + n) for n in ("NONE", "INVALIDATE", "BACKGROUND"))
    assert fills == (capi.FILL_NONE, capi.FILL_INVALIDATE, capi.FILL_BACKGROUND) == (0, 1, 2)
    assert (ref.FILL_NONE, ref.FILL_INVALIDATE, ref.FILL_BACKGROUND) == (0, 1, 2)
    assert abi.define("OFDIS_LR_FUSED_MAX_WIDTH") == capi.LR_FUSED_MAX_WIDTH
    assert abi.define("OFDIS_VERSION") == capi.OFDIS_VERSION == 3
    for name in ("ofdis_batch_flow_mirror", "ofdis_batch_level_flow_mirror", "ofdis_lr_check", "ofdis_disparity_fill",
                 "ofdis_batch_upsample_lr"):
        assert name in capi.ABI_SYMBOLS and hasattr(capi.lib(), name)


def test_create_ex_flag_rules():
    L = capi.lib()
    p = oppoint(2, 256, 112)
    st = p.copy(selectmode=2)
    h = C.c_void_p()
    for mode in (0, 1):
        assert L.ofdis_batch_create_ex(C.byref(h), C.byref(p.copy(selectmode=mode)), 2, capi.BATCH_STEREO_LR) == -1  # INVALID
        assert not h.value
    assert "selectmode 2" in L.ofdis_last_error().decode()
    for flags in (capi.BATCH_REVERSE, capi.BATCH_REVERSE | capi.BATCH_STEREO_LR):
        assert L.ofdis_batch_create_ex(C.byref(h), C.byref(st), 2, flags) == -2  # UNSUPPORTED
        assert not h.value
    for flags in (4, 6, 8, 0x80000000, 0x80000002):
        for params in (p, st):
            assert L.ofdis_batch_create_ex(C.byref(h), C.byref(params), 2, flags) == -1
            assert not h.value


def test_entry_points_without_a_context():
    L = capi.lib()
    assert not L.ofdis_batch_flow_mirror(None)
    assert not L.ofdis_batch_level_flow_mirror(None, 0)
    assert L.ofdis_batch_upsample_lr(None, 0, 1, None, None, None, None, 0, 16, 16, 0.01, 0.5, None) == -1


@pytest.mark.parametrize("alpha,beta", [(-0.01, 0.5), (0.01, -0.5), (math.inf, 0.5), (0.01, math.inf), (math.nan, 0.5),
                                        (0.01, math.nan)])
def test_lr_check_rejects_bad_constants(alpha, beta):
    """(host buffers stand in for the device arrays: the call returns before it would launch)"""
    L = capi.lib()
    f = np.zeros((1, 4, 4), np.float32)
    m = np.zeros((1, 4, 4), np.uint8)
    assert L.ofdis_lr_check(f.ctypes.data, f.ctypes.data, m.ctypes.data, 1, 4, 4, alpha, beta, None) == -1
    assert "alpha" in L.ofdis_last_error().decode()


@pytest.mark.parametrize("n,w,h", [(0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 1 << 16, 1 << 16)])
def test_bad_sizes(n, w, h):
    L = capi.lib()
    f = np.zeros(8, np.float32)
    assert L.ofdis_lr_check(f.ctypes.data, f.ctypes.data, f.ctypes.data, n, w, h, 0.01, 0.5, None) == -1
    assert L.ofdis_lr_check(None, f.ctypes.data, f.ctypes.data, 1, 1, 1, 0.01, 0.5, None) == -1
    for mode in (0, 1, 2):
        assert L.ofdis_disparity_fill(f.ctypes.data, f.ctypes.data, f.ctypes.data, n, w, h, mode, None) == -1
        assert L.ofdis_disparity_fill(f.ctypes.data, None, f.ctypes.data, 1, 1, 1, mode, None) == -1


@pytest.mark.parametrize("mode", [-1, 3, 7, 1 << 20])
def test_fill_rejects_bad_mode(mode):
    L = capi.lib()
    f = np.zeros(16, np.float32)
    assert L.ofdis_disparity_fill(f.ctypes.data, f.ctypes.data, f.ctypes.data, 1, 4, 4, mode, None) == -1
    assert "fill mode" in L.ofdis_last_error().decode()


# ------------------------------------------------------------------------------------ the restatement itself
def test_restatement_hand_built_rows():
    inf = np.float32(np.inf)
    d = np.array([[-3, -1, -7, -2, -9, -4, -5, -6]], np.float32)
    C0, X = ref.CONSISTENT, ref.INCONSISTENT
    fill = lambda m: ref.disparity_fill(d, np.array([m], np.uint8), ref.FILL_BACKGROUND)[0].tolist()
    assert fill([X, X, C0, C0, X, C0, X, X]) == [-7, -7, -7, -2, -2, -4, -4, -4]          # runs touching both borders
    assert fill([X, X, X, C0, X, X, X, X]) == [-2] * 8                                      # a single consistent pixel
    assert fill([X] * 8) == d[0].tolist()                                                    # none: unchanged
    t = np.array([[-5, 0, 0, 5]], np.float32)
    assert ref.disparity_fill(t, np.array([[C0, X, 2, C0]], np.uint8), ref.FILL_BACKGROUND)[0].tolist() == [-5, -5, -5, 5]  # tie: left
    inv = ref.disparity_fill(d, np.array([[X, C0] * 4], np.uint8), ref.FILL_INVALIDATE)[0]
    assert inv.tolist() == [inf, -1, inf, -2, inf, -4, inf, -6]
    # the check: two views of a fronto-parallel plane agree; a pixel whose match lies outside is OUTSIDE
    L, R = np.full((1, 16), -4, np.float32), np.full((1, 16), 4, np.float32)
    assert ref.lr_check(L, R)[0].tolist() == [ref.OUTSIDE] * 4 + [C0] * 12
    assert ref.lr_check(R, L)[0].tolist() == [C0] * 12 + [ref.OUTSIDE] * 4
    R[0, 6] = 9  # one wrong right-view pixel flags the left pixel that lands on it (x - 4 = 6; integer targets: ax = 0)
    assert ref.lr_check(L, R)[0].tolist() == [ref.OUTSIDE] * 4 + [C0] * 6 + [X] + [C0] * 5
    assert ref.lr_check(np.array([[np.nan, 0.0]], np.float32), np.zeros((1, 2), np.float32))[0].tolist() == [ref.OUTSIDE, C0]


def middlebury_lr(flow_of, opp):
    """(DL, DR, ground-truth disparity) at full resolution for the Middlebury pair, gray: flow_of(p, pyr_a, pyr_b) -> level disparity."""
    pr = natural.pair("motorcycle")
    if pr is None:
        pytest.skip("natural pair 'motorcycle' is not available here (tests/natural.py)")
    a, b, truth = pr
    h, w = a.shape[:2]
    p = oppoint(opp, w, h, noc=1).copy(selectmode=2)
    ia, ib = natural.to_channels(a, 1), natural.to_channels(b, 1)
    O = oracle.c_oracle()

    def full(low):
        return O.upsample_crop(p.copy(selectmode=0), np.concatenate([low, low], -1), w, h)[..., 0]
    dl = full(flow_of(p, O.build_pyramid(p, ia), O.build_pyramid(p, ib)))
    dm = full(flow_of(p, O.build_pyramid(p, ref.mirror(ib)), O.build_pyramid(p, ref.mirror(ia))))
    return dl, ref.right_view(dm), truth["disparity"]


def assert_lr_inequalities(dl, dr, gt, what):
    """The issue's statements about a left-right result on the Middlebury pair (alpha 0.01, beta 0.5); prints each figure."""
    ml, mr = ref.lr_check(dl, dr, ALPHA, BETA), ref.lr_check(dr, dl, ALPHA, BETA)
    share_l, share_r = float((ml == 0).mean()), float((mr == 0).mean())
    known = np.isfinite(gt)
    err = np.abs(dl + gt)
    med_c, med_all, med_f = (float(np.median(err[known & (ml == 0)])), float(np.median(err[known])),
                             float(np.median(err[known & (ml != 0)])))
    filled = ref.disparity_fill(dl, ml, ref.FILL_BACKGROUND)
    err_f = np.abs(filled + gt)
    bad0, bad1 = float((err[known] > 2).mean()), float((err_f[known] > 2).mean())
    empty_rows = int((~(ml == 0).any(axis=1)).sum() + (~(mr == 0).any(axis=1)).sum())
    print(f"{what}: consistent {share_l:.3f} / {share_r:.3f}; median |err| consistent {med_c:.2f} < all {med_all:.2f} < flagged "
          f"{med_f:.2f} px; > 2 px off {bad0:.3f} -> {bad1:.3f} after the fill; rows without a consistent pixel {empty_rows}")
    assert share_l >= 0.85 and share_r >= 0.85
    assert med_c < med_all < med_f
    assert bad1 <= bad0
    assert empty_rows == 0
    assert (dl <= 0).all() and (dr >= 0).all()


@pytest.mark.parametrize("opp", [2, 3])
def test_restatement_on_the_reference_build(opp):
    """Measured with the reference build: consistent 0.907 / 0.894 (operating point 2) and 0.915 / 0.909 (3); median error
    1.47 < 1.62 < 8.79 px and 0.29 < 0.33 < 7.28 px; more than 2 px off 0.431 -> 0.426 and 0.196 -> 0.184 after the fill."""
    R = oracle.need_ref("de_int", True)
    if R is None:
        pytest.skip("comparison against the compiled reference skipped: neither /root/reference nor oracle/_ref exists here")
    dl, dr, gt = middlebury_lr(lambda p, pa, pb: R.flow(p, pa[0], pa[1], pa[2], pb[0]), opp)
    assert_lr_inequalities(dl, dr, gt, f"reference build, operating point {opp}")
