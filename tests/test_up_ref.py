"""tests/up_ref.py (the numpy statement of the level flow at full resolution for a free UpGeom) against what already pins that
step without a GPU -- the C restatement (oracle_upsample_crop) and the exact Fraction hand vectors of tests/test_upsample_pin.py
-- and the conditions on the planted level flows of tests/test_gpu_level_routes.py, asserted here on the reference alone."""
import numpy as np
import pytest

from of_dis_amd import gmotion
from of_dis_amd.params import oppoint
from test_upsample_pin import PIN_CASES, _case, _exact_f32, _hand_upsample
from trajfilter_cases import fb_mask_ref
from up_ref import CROP_ABOVE_S, EXACT_T, GEOM_IDS, GEOMS, NPAIRS, exact_masks, geom, level_flows, up_ref, up_ref1

_f32 = np.float32
ALPHA, BETA = 0.01, 0.5


def _bits(a):
    return np.ascontiguousarray(a, _f32).view(np.uint32)


def _geom_of(p, w, h):
    g = geom(p.width >> p.sc_l, p.height >> p.sc_l, p.sc_l, w, h)
    assert g[3:5] == ((p.width - w) // 2, (p.height - h) // 2)
    return g


@pytest.mark.parametrize("w,h,lv", PIN_CASES)
def test_up_ref_equals_the_oracle_on_the_pin_cases(orc, w, h, lv):
    p, flow, _, _ = _case(w, h, lv, 31 + w)
    g = _geom_of(p, w, h)
    flow = (np.random.default_rng(977 + w).standard_normal(flow.shape) * 3).astype(_f32)
    assert np.array_equal(_bits(up_ref(flow, g)), _bits(orc.upsample_crop(p, flow, w, h)))


@pytest.mark.parametrize("w,h,op", [(1024, 436, 2), (333, 251, 1), (320, 240, 3)])
def test_up_ref_equals_the_oracle_at_operating_points(orc, w, h, op):
    p = oppoint(op, w, h)
    g = _geom_of(p, w, h)
    flow = (np.random.default_rng(w).standard_normal((g[1], g[0], 2)) * 3).astype(_f32)
    assert np.array_equal(_bits(up_ref(flow, g)), _bits(orc.upsample_crop(p, flow, w, h)))


@pytest.mark.parametrize("w,h,lv", PIN_CASES)
def test_up_ref_equals_the_hand_vectors_on_the_pin_cases(w, h, lv):
    p, flow, left, top = _case(w, h, lv, 31 + w)
    g = _geom_of(p, w, h)
    expect = _exact_f32(_hand_upsample(flow, 1 << lv, left, top, w, h))
    assert np.array_equal(_bits(up_ref(flow, g)), _bits(expect))
    assert np.array_equal(_bits(up_ref1(flow[..., 1], g)), _bits(expect[..., 1]))   # (one channel: the same values)


# the geometries no operating point produces: sw == 1, sh == 1, both, and a crop larger than s
OFF_GRID = [g for g in GEOMS if g[0] == 1 or g[1] == 1] + [CROP_ABOVE_S]


@pytest.mark.parametrize("g", OFF_GRID, ids=[f"{g[0]}x{g[1]}-x{1 << g[2]}-{g[5]}x{g[6]}" for g in OFF_GRID])
def test_up_ref_equals_hand_vectors_off_the_operating_points(g):
    """the same exact rational arithmetic on small integers, for the level sizes and crops the pin cases cannot reach"""
    sw, sh, sc_l, left, top, wo, ho = g
    assert OFF_GRID.count(g) == 1 and len(OFF_GRID) == 5
    flow = np.random.default_rng(5 + 10 * sw + sh).integers(-9, 10, (sh, sw, 2)).astype(_f32)
    expect = _exact_f32(_hand_upsample(flow, 1 << sc_l, left, top, wo, ho))
    assert np.array_equal(_bits(up_ref(flow, g)), _bits(expect))
    if sw == 1 and sh == 1:
        assert (expect == flow[0, 0] * _f32(1 << sc_l)).all()
    if g == CROP_ABOVE_S:   # column 0 of the crop is padded column 3: between level columns 1 and 2, never 0
        assert left > 1 << sc_l and top > 1 << sc_l
        other = flow.copy()
        other[:, 0], other[0, :] = 99, 99
        assert np.array_equal(up_ref(other, g), up_ref(flow, g))


def test_up_ref_takes_frames_on_leading_axes():
    g = GEOMS[4]
    fw, _ = level_flows(g, "coherent")
    assert np.array_equal(_bits(up_ref(fw, g)), _bits(np.stack([up_ref(f, g) for f in fw])))


# ------------------------------------------------------------------ the planted level flows (tests/test_gpu_level_routes.py)
def _masks(g, family):
    fw, rev = level_flows(g, family)
    ufw, urev = up_ref(fw, g), up_ref(rev, g)
    return fb_mask_ref(ufw, urev, ALPHA, BETA), fb_mask_ref(urev, ufw, ALPHA, BETA)


def test_every_code_occurs_in_the_reference_masks():
    seen = set()
    for g in GEOMS:
        for family in ("wild", "coherent"):
            for m in _masks(g, family):
                seen |= set(np.unique(m).tolist())
    assert seen == {0, 1, 2}, seen


def test_the_wild_family_has_nan_beside_finite_values():
    """per geometry of a dozen level pixels or more (2 % of the family's values are NaN and 4 % infinite: a level of four pixels
    may have none): a poisoned group and, beside it, finite values"""
    for g in GEOMS:
        u = up_ref(level_flows(g, "wild")[0], g)
        if g[0] * g[1] >= 12:
            assert np.isnan(u).any() and np.isfinite(u).any(), g
    assert sum(int(np.isnan(up_ref(level_flows(g, "wild")[0], g)).sum()) for g in GEOMS) > 1000


@pytest.mark.parametrize("g", GEOMS, ids=GEOM_IDS)
def test_the_exact_family_is_t_at_every_pixel_and_its_masks_are_the_closed_form(g):
    fw, rev = level_flows(g, "exact")
    ufw, urev = up_ref(fw, g), up_ref(rev, g)
    for k, t in enumerate(EXACT_T):
        assert (ufw[k] == np.asarray(t, _f32)).all() and (urev[k] == -np.asarray(t, _f32)).all(), (g, k)
    want = exact_masks(g)
    got = _masks(g, "exact")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    wo, ho = g[5], g[6]
    if wo > 3 and ho > 2:   # targets exactly on the last column / row are inside: pair 0 moves (1, -1), pair 1 (-3, 2)
        assert want[0][0][1, wo - 2] == 0 and want[0][0][1, wo - 1] == 2 and want[0][1][ho - 3, 3] == 0
    assert (want[0][2] == 2).all() and (want[0][3] == 0).all()


def test_the_coherent_family_gives_full_fits():
    """a geometry of 30 or more pixels fits all 6 parameters (status GM_OK_AFFINE) and all 8 (stats[:, 2] == 8) in at least one
    pair, under the forward mask"""
    for g in GEOMS:
        if g[5] * g[6] < 30:
            continue
        fw, rev = level_flows(g, "coherent")
        ufw = up_ref(fw, g)
        mask = _masks(g, "coherent")[0]
        _, s6 = gmotion.global_motion_ref(ufw, mask, gmotion.GM_AFFINE, 3, 1.0)
        _, s8 = gmotion.projective_motion_ref(ufw, mask, 3, 1.0)
        assert (s6[:, 2] == gmotion.GM_OK_AFFINE).any() and (s6[:, 0] >= 3).any(), (g, s6)
        assert (s8[:, 2] == 8).any(), (g, s8)
    assert NPAIRS == 4
