"""Which kernel classes one pass launches on each route of the TV refinement (ofdis_schedule.hip: plan_level).

Under the exact contract every route gives the same bits, so the bit-exact tests cannot tell a misrouted level from a right
one: a level that silently loses its fused route still passes them.  These cases pin, per kernel class of capi.K_NAMES, how
many launches a pass makes.  Random 8-bit frames through the on-device pyramid: the counts do not depend on the content.

The second group of cases runs the arms of the core launchers' own kernel choice that those routes leave out (patch kernels by
geometry, cost function and knob; tv_prep by level width; tall and one-frame fused TV).  A count per class does not say which
instantiation ran: the patch choice itself is held on the host by tests/test_patch_kernel_choice.py.
"""
import numpy as np
import pytest

from of_dis_amd.params import oppoint

pytestmark = pytest.mark.gpu

GRAY = (1024, 436, 1)
RGB_SMALL = (320, 240, 3)
STEREO = (1242, 375, 1)
WIDE = {"sc_f": 4, "sc_l": 3}

# id: (frame size and channels, operating point, frames, params changed, knobs at creation, knobs set after creation, reverse)
CASES = {
    "gray":                   (GRAY, 2, 4, {}, {}, {}, False),
    "gray_no_prep_densify":   (GRAY, 2, 4, {}, {"prep_densify": 0}, {}, False),
    "gray_no_finish_fusion":  (GRAY, 2, 4, {}, {"finish_fusion": 0}, {}, False),
    "gray_fused_tv_off":      (GRAY, 2, 4, {}, {"fused_tv": 0}, {}, False),
    "gray_fused_tv_off_late": (GRAY, 2, 4, {}, {}, {"fused_tv": 0}, False),
    "gray_fbcon":             (GRAY, 2, 4, {"usefbcon": 1}, {}, {}, False),
    "gray_no_tvref":          (GRAY, 2, 4, {"usetvref": 0}, {}, {}, False),
    "gray_reverse":           (GRAY, 2, 4, {}, {}, {}, True),
    "gray_op3_records":       (GRAY, 3, 4, {}, {"fused_rgb_min": 1}, {}, False),
    "gray_op3_per_stage":     (GRAY, 3, 4, {}, {"fused_rgb_min": 1 << 30}, {}, False),
    "rgb_exact":              ((1024, 436, 3), 2, 4, {}, {"contract": 0}, {}, False),
    "rgb_exact_forced":       ((1024, 436, 3), 2, 4, {}, {"contract": 0, "fused_rgb_min": 1}, {}, False),
    "rgb_fused_15":           (RGB_SMALL, 2, 15, {}, {"contract": 1}, {}, False),
    "rgb_fused_16":           (RGB_SMALL, 2, 16, {}, {"contract": 1}, {}, False),
    "stereo_exact":           (STEREO, 2, 1, {"selectmode": 2}, {"contract": 0}, {}, False),
    "stereo_exact_forced":    (STEREO, 2, 1, {"selectmode": 2}, {"contract": 0, "fused_rgb_min": 1}, {}, False),
    "stereo_fused":           (STEREO, 2, 1, {"selectmode": 2}, {"contract": 1}, {}, False),
    # the arms of the core launchers' kernel choice (choose_patch_kernel, launch_tv_prep, launch_tv_fused_tall, tv_fused_mode)
    "rgb_op3_pixel_weights":  (RGB_SMALL, 3, 2, {}, {"contract": 0}, {}, False),
    "rgb_op2_lanes16":        (RGB_SMALL, 2, 2, {}, {"contract": 0}, {}, False),
    "gray_no_gray8":          (GRAY, 2, 4, {}, {"gray8": 0}, {}, False),
    "rgb_op3_no_rgb12":       (RGB_SMALL, 3, 2, {}, {"contract": 0, "rgb12": 0}, {}, False),
    "rgb_op3_lpp32":          (RGB_SMALL, 3, 2, {}, {"contract": 0, "rgb12_lpp": 32}, {}, False),
    "gray_costfct1":          (GRAY, 2, 4, {"costfct": 1}, {}, {}, False),
    "rgb_op3_costfct2":       (RGB_SMALL, 3, 2, {"costfct": 2}, {"contract": 0}, {}, False),
    "stereo_rgb":             ((1242, 375, 3), 2, 1, {"selectmode": 2}, {"contract": 0}, {}, False),
    # 64 rows leave two levels (the coarsest needs four rows): 96 x 4 and 192 x 8, three wavefronts side by side in tv_prep;
    # 128 x 4 and 256 x 8, four; with and without the densification inside it
    "gray_1536x64":           ((1536, 64, 1), 2, 4, WIDE, {}, {}, False),
    "gray_1536x64_no_prep_densify": ((1536, 64, 1), 2, 4, WIDE, {"prep_densify": 0}, {}, False),
    "gray_2048x64":           ((2048, 64, 1), 2, 4, WIDE, {}, {}, False),
    "gray_2048x64_no_prep_densify": ((2048, 64, 1), 2, 4, WIDE, {"prep_densify": 0}, {}, False),
    "gray_1080p":             ((1920, 1080, 1), 2, 4, {}, {}, {}, False),   # tall levels (more than 64 rows), grouped
    "gray_1080p_ungrouped":   ((1920, 1080, 1), 2, 4, {}, {"fused_tall_group": 0}, {}, False),
    "gray_one_frame":         (GRAY, 2, 1, {}, {}, {}, False),   # the multi-wave modes of the fused TV kernel
}

# launches per pass in the order of capi.K_NAMES: warp, derivatives, tv_system, sor, patch_optimize, densify, tv_finish,
# tv_fused (recorded with the library before the routing was gathered into plan_level)
EXPECTED = {
    "gray":                   ( 0,  3,  0,  0,  3,  0,  0,  3),
    "gray_fbcon":             ( 0,  5,  0,  0,  3,  5,  0,  5),
    "gray_fused_tv_off":      ( 3,  3, 15, 15,  3,  3,  3,  0),
    "gray_fused_tv_off_late": ( 0,  3,  0,  0,  3,  0,  0,  3),
    "gray_no_finish_fusion":  ( 0,  3,  0,  0,  3,  3,  3,  3),
    "gray_no_prep_densify":   ( 0,  3,  0,  0,  3,  3,  0,  3),
    "gray_no_tvref":          ( 0,  0,  0,  0,  3,  3,  0,  0),
    "gray_op3_per_stage":     ( 1,  5,  2,  2,  5,  5,  1,  4),
    "gray_op3_records":       ( 1,  5,  0,  0,  5,  5,  0,  5),
    "gray_reverse":           ( 0,  6,  0,  0,  6,  0,  0,  6),
    "rgb_exact":              ( 3,  3, 15, 15,  3,  3,  3,  0),
    "rgb_exact_forced":       ( 3,  3,  0,  0,  3,  3,  0,  3),
    "rgb_fused_15":           ( 3,  3, 12, 12,  3,  3,  3,  0),
    "rgb_fused_16":           ( 3,  3,  0,  0,  3,  3,  0,  3),
    "stereo_exact":           ( 3,  3, 15, 15,  3,  3,  3,  0),
    "stereo_exact_forced":    ( 3,  3,  0,  0,  3,  3,  3,  3),
    "stereo_fused":           ( 3,  3,  0,  0,  3,  3,  3,  3),
    # (recorded with the library before the core launchers' choices were gathered)
    "gray_1080p":                    ( 0,  3,  0,  0,  3,  0,  0,  3),
    "gray_1080p_ungrouped":          ( 0,  3,  0,  0,  3,  0,  0,  3),
    "gray_1536x64":                  ( 0,  2,  0,  0,  2,  0,  0,  2),
    "gray_1536x64_no_prep_densify":  ( 0,  2,  0,  0,  2,  2,  0,  2),
    "gray_2048x64":                  ( 0,  2,  0,  0,  2,  0,  0,  2),
    "gray_2048x64_no_prep_densify":  ( 0,  2,  0,  0,  2,  2,  0,  2),
    "gray_costfct1":                 ( 0,  3,  0,  0,  3,  0,  0,  3),
    "gray_no_gray8":                 ( 0,  3,  0,  0,  3,  0,  0,  3),
    "gray_one_frame":                ( 0,  3,  0,  0,  3,  0,  0,  3),
    "rgb_op2_lanes16":               ( 3,  3, 12, 12,  3,  3,  3,  0),
    "rgb_op3_costfct2":              ( 4,  4, 10, 10,  4,  4,  4,  0),
    "rgb_op3_lpp32":                 ( 4,  4, 10, 10,  4,  4,  4,  0),
    "rgb_op3_no_rgb12":              ( 4,  4, 10, 10,  4,  4,  4,  0),
    "rgb_op3_pixel_weights":         ( 4,  4, 10, 10,  4,  4,  4,  0),
    "stereo_rgb":                    ( 3,  3, 15, 15,  3,  3,  3,  0),
}


def make_batch(gpu, case):
    """The case's context, created under the current knobs with the case's knobs at creation set by the caller, then the
    case's later knobs; filled with random frames."""
    (w, h, noc), opp, nframes, pchange, _, after, reverse = case
    b = gpu.Batch(oppoint(opp, w, h, noc=noc).copy(**pchange), nframes, reverse=reverse)
    if after:
        gpu.set_tuning(**after)
    rng = np.random.default_rng(11)
    frames = [gpu.Dev(rng.integers(0, 256, (nframes, h, w, noc), dtype=np.uint8)) for _ in range(2)]
    b.build_pyramids_u8(frames[0].ptr, frames[1].ptr, w, h)
    return b, frames


def launch_counts(gpu, case):
    old = gpu.set_tuning(**case[4])
    try:
        b, _frames = make_batch(gpu, case)
        try:
            b.timing(True)
            b.run()
            gpu.check(gpu.lib().ofdis_sync(None))
            return {name: b.kernel_time(k)[1] for k, name in enumerate(gpu.K_NAMES)}
        finally:
            b.close()
    finally:
        gpu.restore_tuning(old)


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_classes_per_pass(gpu, name):
    assert launch_counts(gpu, CASES[name]) == dict(zip(gpu.K_NAMES, EXPECTED[name]))
