"""The lanes where a folded lane shift (ofdis_dev.h: mul_pairs_from_prev, fmac_pairs_from_next, vertical_terms) meets a border
or a lane-group boundary: the first and last row of a frame, the first and last lane of a 16- / 32- / 64-lane group, the
idle lanes behind a short frame and the idle groups of a ragged last wavefront.  A shift folded into its consumer reads
zero at the wavefront's ends and the NEIGHBOURING FRAME's row at a group boundary, exactly like the move it replaces; every
consumer multiplies that by an edge weight that is zero there or selects it away (ofdis_fused.hip, "Border handling").

Gray one-level pyramids with h in {4, 15, 16, 17, 31, 32, 33, 56, 63, 64} and w in {16, 17, 33}; 3 and 5 frames (at
16 / 32 lanes per frame the last lane group of a wavefront is partly or wholly idle); strip lengths 1, 2 (a strip length
must divide the frame count: with 3 and 5 frames a request of 2 falls back to 1, so 4 frames are run as well) and the whole
batch as one strip; 1, 2 and 3 sweeps; brightness term on and off; every mapping of the tv_variant fixture; the tall
kernel at h in {65, 68, 128}; the stereo kernel de_fused_kernel at h in {12, 48}.  Exact contract: bit for bit against the
oracle's varref_level.  Fused contract: the same gray geometries against the PLAIN reference build with the bounds of
tests/test_gpu_contract.py (mean < 1e-4 px, max < 1e-3 px).

Every geometry here went through the oracle on a CPU before it was committed: all flows finite.
"""
import itertools

import numpy as np
import pytest

import gen_synth
import oracle
from common import assert_bits_equal, rand_planes
from of_dis_amd.params import oppoint

pytestmark = pytest.mark.gpu

HEIGHTS = (4, 15, 16, 17, 31, 32, 33, 56, 63, 64)
WIDTHS = (16, 17, 33)
MEAN_BAR, MAX_BAR = 1e-4, 1e-3  # tests/test_gpu_contract.py


def _gray_cases():
    """(w, h, frames, tv_innerit, tv_solverit, tv_delta): per height both frame counts, all three sweep counts and the
    brightness term on and off; two or three fixed-point iterations, so that the iteration-pipelined mappings apply."""
    out = []
    for idx, (h, w) in enumerate(itertools.product(HEIGHTS, WIDTHS)):
        out.append((w, h, (3, 5)[idx % 2], 2 + (idx // 3) % 2, 1 + idx % 3, (5.0, 0.0)[(idx // 2) % 2]))
    out += [(17, 16, 4, 2, 3, 5.0), (33, 33, 4, 3, 2, 0.0), (16, 63, 4, 2, 1, 5.0)]  # strips of two frames
    return out


TALL_CASES = [(17, 65, 3, 2, 3, 5.0), (33, 68, 5, 3, 1, 0.0), (16, 128, 3, 2, 2, 5.0), (33, 65, 5, 1, 3, 0.0)]
STEREO_CASES = [(17, 12, 3, 2, 3), (33, 12, 5, 3, 1), (16, 48, 5, 2, 2), (33, 48, 3, 1, 3)]

_cache = {}


def _level(w, h, nfr, innerit, solverit, delta, selectmode=0):
    """One-level pyramid of free size (tests/test_gpu_kernels.py::test_varref_levels_of_65_to_128_rows' construction):
    (p, im_a [nfr, ...], im_b, flows [nfr, h, w, 2 or 1]); frame k uses pair k % 2 and an incoming flow of its own."""
    key = (w, h, nfr, innerit, solverit, delta, selectmode)
    if key not in _cache:
        O = oracle.c_oracle()
        p = oppoint(2, w, h).copy(sc_f=0, sc_l=0, p_samp_s=4, imgpadding=4, tv_innerit=innerit, tv_solverit=solverit,
                                  tv_delta=delta, selectmode=selectmode)
        p.width, p.height = w, h
        rng = np.random.default_rng(w * 1000 + h)
        pairs = [gen_synth.make_pair(w, h, 700 + k, 1) for k in range(2)]
        if selectmode == 2:  # second image as the left camera (tests/test_gpu_stereo.py)
            pyr = [(O.build_pyramid(p, ib), O.build_pyramid(p, ia)) for ia, ib, _ in pairs]
            flows = [-np.abs(rand_planes(rng, h, w, 1, scale=1.5)) for _ in range(nfr)]
            for f in flows:
                f[::7, ::5] = 0.3
            flows[1][h - 1, w - 1] = -3.0 * w
        else:
            pyr = [(O.build_pyramid(p, ia), O.build_pyramid(p, ib)) for ia, ib, _ in pairs]
            flows = [rand_planes(rng, h, w, 2, scale=(1.5, 0.3, 5.0, 1.0)[f % 4]) for f in range(nfr)]
            flows[2][h - 1, w - 1] = (2.5 * w, -2.5 * h)  # far outside the image: mask 0, clamped taps
            flows[1][0, 0] = (-2.5 * w, 2.5 * h)
        im_a = np.stack([pyr[f % 2][0][0][0] for f in range(nfr)])
        im_b = np.stack([pyr[f % 2][1][0][0] for f in range(nfr)])
        _cache[key] = (p, im_a, im_b, np.stack(flows))
    return _cache[key]


def _reference(R, tag, key):
    """varref_level of every frame through the reference R, computed once per geometry and shared (never modified)."""
    if (tag, key) not in _cache:
        p, im_a, im_b, flows = _level(*key)
        refs = np.stack([R.varref_level(p, 0, im_a[f], im_b[f], flows[f]) for f in range(len(flows))])
        assert np.isfinite(refs).all(), key
        refs.setflags(write=False)
        _cache[(tag, key)] = refs
    return _cache[(tag, key)]


def _strips(nfr):
    return (1, 2, nfr)


def test_gray_levels_bit_exact(gpu, orc, tv_variant):
    for case in _gray_cases():
        key = case + (0,)
        p, im_a, im_b, flows = _level(*key)
        refs = _reference(orc, "oracle", key)
        for strip in _strips(case[2]):
            old = gpu.set_tuning(fused_strip=strip)
            try:
                got = gpu.varref_level(p, 0, im_a, im_b, flows)
            finally:
                gpu.restore_tuning(old)
            for f in range(case[2]):
                assert_bits_equal(got[f], refs[f], f"{tv_variant} strip {strip} {case} frame {f}")


@pytest.mark.parametrize("knobs", [{}, {"fused_strip": 1}, {"fused_tall_group": 0}])
def test_tall_levels_bit_exact(gpu, orc, knobs):
    old = gpu.set_tuning(**knobs)
    try:
        for case in TALL_CASES:
            key = case + (0,)
            p, im_a, im_b, flows = _level(*key)
            refs = _reference(orc, "oracle", key)
            got = gpu.varref_level(p, 0, im_a, im_b, flows)
            for f in range(case[2]):
                assert_bits_equal(got[f], refs[f], f"tall {knobs} {case} frame {f}")
    finally:
        gpu.restore_tuning(old)


def test_stereo_fused_levels_bit_exact(gpu):
    """de_fused_kernel (levels of at most 64 rows forced onto it: ofdis_tuning.fused_rgb_min = 1) against the reference
    compiled in stereo mode with the wave64 summation order."""
    R = oracle.need_ref("de_int", True)
    assert R is not None, "the stereo reference build oracle/_ref/libofdis_ref_de_int_w64.so is not on this machine"
    old = gpu.set_tuning(fused_rgb_min=1)
    try:
        for w, h, nfr, innerit, solverit in STEREO_CASES:
            key = (w, h, nfr, innerit, solverit, 5.0, 2)
            p, im_a, im_b, flows = _level(*key)
            refs = _reference(R, "de", key)
            got = gpu.varref_level(p, 0, im_a, im_b, flows)
            for f in range(nfr):
                assert_bits_equal(got[f], refs[f], f"stereo {key} frame {f}")
    finally:
        gpu.restore_tuning(old)


def test_gray_levels_fused_contract(gpu, tv_variant):
    """The fused contract on the same geometries against the plain (sequential-sum) reference build."""
    R = oracle.need_ref("int", False)
    assert R is not None, "the plain reference build oracle/_ref/libofdis_ref_int.so is not on this machine"
    worst = (0.0, 0.0, None)
    bad = []
    old = gpu.set_tuning(contract=1)
    try:
        for case in _gray_cases():
            key = case + (0,)
            p, im_a, im_b, flows = _level(*key)
            refs = _reference(R, "plain", key)
            got = gpu.varref_level(p, 0, im_a, im_b, flows)
            assert np.isfinite(got).all(), case
            epe = np.sqrt(((got.astype(np.float64) - refs) ** 2).sum(-1))
            for f in range(case[2]):
                m, x = float(epe[f].mean()), float(epe[f].max())
                if x > worst[1]:
                    worst = (m, x, (case, f))
                if not (m < MEAN_BAR and x < MAX_BAR):
                    bad.append((case, f, m, x))
    finally:
        gpu.restore_tuning(old)
    print(f"{tv_variant}: worst frame mean {worst[0]:.2e} max {worst[1]:.2e} px at {worst[2]}")
    assert not bad, bad[:5]
