"""-m gpu: every level-flow finish kernel held to the definition at factors x1 to x16, on planted level flows and a free UpGeom.

A context reaches the level forms only at a few sizes (x1, x2) and on the smooth flows of a real estimation.  Here every level
launcher is called through the launch hooks (tests/launch_hooks.py) at the product's launch limits, on the geometries of
tests/up_ref.py (GEOMS: every factor, the clamped half groups at all four borders, crops above s/2, levels 1 wide or 1 high,
wo < 4, wo % 4 != 0, ho == 1) and three families of level flows (level_flows: wild, coherent, exact), four pairs each.

  a. upsample_crop (one and two channels) and the two flows of upsample_bidir against up_ref: the same bit patterns wherever
     the reference is not NaN, NaN exactly where it is (payloads and signs of NaN are not compared: x86 and the GPU make
     different default NaNs for inf * 0).
  b. the two masks of upsample_bidir against fb_mask_ref (tests/trajfilter_cases.py) on the device's own flows of (a), and for
     the exact family against the closed form.
  c. every other level route against its frames form -- the product's public standalone call -- on the materialised outputs of
     (a) and (b): byte for byte, models and stats as raw 64-bit patterns, residuals with their NaN payloads (both sides are the
     GPU).
  d. the frames form against its numpy definition on those same inputs, for every geometry of up to 1024 output pixels and for
     the wild family of 96x61: with (a) this closes the chain on numpy.
  e. every output through Out (0xAB prefill, a guard behind it, no frame left unwritten); the byte outputs of the quad kernels
     once more at offsets 1 and 2 into their buffers, where quad_vec is false.

Dense trajectories write only the slots below info[0], so their arrays are the binding's own (as tests/test_gpu_dense_tracks.py
reads them), and their frames form rejects a side below the stride: the two geometries 1 pixel wide or high are not run there.
Conditions on the planted inputs are asserted on the reference in tests/test_up_ref.py, without a GPU."""
import numpy as np
import pytest

import stereo_lr_ref
from launch_hooks import hooks, launch, upsample_lr_fuses
from of_dis_amd import gmotion, tracking
from of_dis_amd.temporal import temporal_filter_ref, trajectory_filter_ref, trajectory_weights
from test_gpu_dense_tracks import _threshold, assert_dense_equal
from test_gpu_interp import ref_frames
from test_gpu_launch_limits import AB, Out, assert_all_same, assert_same_bytes, img_shape, sync
from trajfilter_cases import fb_mask_ref, random_case
from up_ref import CROP_ABOVE_S, EXACT_T, FAMILIES, GEOM_IDS, GEOMS, NPAIRS, exact_masks, level_flows, up_ref, up_ref1

pytestmark = pytest.mark.gpu
_f32 = np.float32
ALPHA, BETA = 0.01, 0.5
TIMES = np.array([0.5, 0.0, 1.0, 0.3], _f32)
WEIGHTS = trajectory_weights(2, 0.75)
TAU, WN = 24.0, 0.75
GM_ROUNDS, GM_THRESH = 3, 1.0
ENC_F32 = 0
CASES = [pytest.param(g, family, id=f"{gid}-{family}") for g, gid in zip(GEOMS, GEOM_IDS) for family in FAMILIES]
UP_CASES = CASES + [pytest.param(CROP_ABOVE_S, family, id=f"crop-above-s-{family}") for family in FAMILIES]
by_case = pytest.mark.parametrize("g,family", CASES)


@pytest.fixture(autouse=True)
def product_limits():
    """every launch here is the product's: the test library's two launch limits at the product's values"""
    hooks().ofdis_test_set_launch_limits(0, 0)


def with_definition(g, family):
    """(d) runs for every geometry of up to 1024 output pixels, and for the wild family of the largest one"""
    return g[5] * g[6] <= 1024 or family == "wild"


def frames_of(g, noc):
    """five "smooth" frames of wo x ho (a ramp plus noise: the filters' intensity gates let neighbours in)"""
    return random_case(NPAIRS, g[5], g[6], noc, "smooth")[0]


def assert_bits_or_nan(got, want, what):
    """float32 arrays: NaN exactly where `want` is NaN, the same bit patterns elsewhere"""
    assert got.shape == want.shape and got.dtype == want.dtype == _f32, (what, got.shape, want.shape)
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        bad = np.argwhere(np.isnan(got) != nan)
        raise AssertionError(f"{what}: NaN in {len(bad)} of {got.size} places where the reference has none or the reverse; "
                             f"first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")
    same = (got.view(np.uint32) == want.view(np.uint32)) | nan
    if not same.all():
        bad = np.argwhere(~same)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ; first at {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")


def at_offsets(gpu, want, what, call):
    """the byte outputs `want` once more at offsets 1 and 2 into their buffers: call(*pointers) launches; the same bytes, nothing
    written before or behind them"""
    for off in (1, 2):
        outs = [Out(gpu, (1, w.size + off)) for w in want]
        call(*[o.ptr + off for o in outs])
        sync(gpu)
        for k, (o, w) in enumerate(zip(outs, want)):
            raw = o.get(f"{what}, output {k} at offset {off}")[0]
            assert (raw[:off] == AB).all(), f"{what}, output {k}: written before the array at offset {off}"
            assert np.array_equal(raw[off:], w.reshape(-1)), f"{what}, output {k} at offset {off}: the bytes differ"


_MATERIALISED = {}


def materialised(gpu, g, family):
    """(ufw, urev, mask_fw, mask_rev) of launch_upsample_bidir on the planted level flows: the inputs of every frames form,
    computed once per case and read-only"""
    if (g, family) not in _MATERIALISED:
        fw, rev = level_flows(g, family)
        wo, ho = g[5], g[6]
        dfw, drev = gpu.Dev(fw), gpu.Dev(rev)
        outs = [Out(gpu, (NPAIRS, ho, wo, 2), _f32), Out(gpu, (NPAIRS, ho, wo, 2), _f32), Out(gpu, (NPAIRS, ho, wo)),
                Out(gpu, (NPAIRS, ho, wo))]
        launch("upsample_bidir", dfw.ptr, drev.ptr, *[o.ptr for o in outs], NPAIRS, *g, ALPHA, BETA)
        sync(gpu)
        arrays = tuple(o.get(f"upsample_bidir output {k}") for k, o in enumerate(outs))
        for a in arrays:
            a.setflags(write=False)
        _MATERIALISED[(g, family)] = arrays
    return _MATERIALISED[(g, family)]


def level_devs(gpu, g, family):
    fw, rev = level_flows(g, family)
    return gpu.Dev(fw), gpu.Dev(rev)


# ------------------------------------------------------------------ a, b: the upsample itself
def _crop(gpu, level, g, channels):
    d = gpu.Dev(level)
    out = Out(gpu, (level.shape[0], g[6], g[5], channels), _f32)
    launch("upsample_crop_enc", d.ptr, out.ptr, level.shape[0], *g, channels, ENC_F32, 1.0, 0.0)
    sync(gpu)
    return out.get(f"upsample_crop, {channels} channels")


@pytest.mark.parametrize("g,family", UP_CASES)
def test_upsample_against_up_ref_and_masks_against_the_definition(gpu, g, family):
    fw, rev = level_flows(g, family)
    want_fw, want_rev = up_ref(fw, g), up_ref(rev, g)
    assert_bits_or_nan(_crop(gpu, fw, g, 2), want_fw, "upsample_crop, two channels")
    one = np.ascontiguousarray(rev[..., 1])
    assert_bits_or_nan(_crop(gpu, one, g, 1)[..., 0], up_ref1(one, g), "upsample_crop, one channel")
    ufw, urev, mf, mr = materialised(gpu, g, family)
    assert_bits_or_nan(ufw, want_fw, "upsample_bidir, forward flow")
    assert_bits_or_nan(urev, want_rev, "upsample_bidir, reverse flow")
    assert_same_bytes(mf, fb_mask_ref(ufw, urev, ALPHA, BETA), "upsample_bidir, forward mask")
    assert_same_bytes(mr, fb_mask_ref(urev, ufw, ALPHA, BETA), "upsample_bidir, reverse mask")
    if family == "exact":
        closed = exact_masks(g)
        assert_same_bytes(mf, closed[0], "forward mask, closed form")
        assert_same_bytes(mr, closed[1], "reverse mask, closed form")
        for k, t in enumerate(EXACT_T):
            assert (ufw[k] == np.asarray(t, _f32)).all(), (k, t)


# ------------------------------------------------------------------ c, d, e: the level routes
@by_case
def test_interp_bidir(gpu, g, family):
    ufw, urev, mf, mr = materialised(gpu, g, family)
    dfw, drev = level_devs(gpu, g, family)
    wo, ho = g[5], g[6]
    for noc in (1, 3):
        frames = frames_of(g, noc)
        A, B = np.ascontiguousarray(frames[:-1]), np.ascontiguousarray(frames[1:])
        da, db = gpu.Dev(A), gpu.Dev(B)
        shape = (NPAIRS, TIMES.size) + img_shape(NPAIRS, wo, ho, noc)[1:]

        def call(ptr):
            launch("interp_bidir", da.ptr, db.ptr, dfw.ptr, drev.ptr, ptr, NPAIRS, *g, noc, TIMES.ctypes.data, TIMES.size, ALPHA, BETA)

        out = Out(gpu, shape)
        call(out.ptr)
        sync(gpu)
        got = out.get("interp_bidir out")
        want = gpu.interpolate(A, B, ufw, urev, TIMES, mf, mr)
        assert_same_bytes(got, want, f"interp_bidir vs ofdis_interpolate, noc {noc}")
        if with_definition(g, family):
            assert_same_bytes(want, ref_frames(A, B, ufw, urev, mf, mr, TIMES), f"ofdis_interpolate vs interp_ref, noc {noc}")
        at_offsets(gpu, [want], f"interp_bidir, noc {noc}", call)


@by_case
def test_tfilter_level(gpu, g, family):
    ufw, urev, mf, mr = materialised(gpu, g, family)
    dfw, drev = level_devs(gpu, g, family)
    wo, ho = g[5], g[6]
    for noc in (1, 3):
        frames = frames_of(g, noc)
        df = gpu.Dev(frames)

        def call(out_ptr, sup_ptr):
            launch("tfilter_level", df.ptr, dfw.ptr, drev.ptr, out_ptr, sup_ptr, NPAIRS, *g, noc, WN, TAU, ALPHA, BETA)

        out, sup = Out(gpu, img_shape(NPAIRS + 1, wo, ho, noc)), Out(gpu, (NPAIRS + 1, ho, wo))
        call(out.ptr, sup.ptr)
        sync(gpu)
        got = out.get("tfilter_level out"), sup.get("tfilter_level support")
        want = gpu.temporal_filter(frames, ufw, urev, mf, mr, wn=WN, tau=TAU)
        assert_all_same(got, want, f"tfilter_level vs ofdis_temporal_filter, noc {noc}", ["out", "support"])
        if with_definition(g, family):
            assert_all_same(want, temporal_filter_ref(frames, ufw, urev, mf, mr, WN, TAU),
                            f"ofdis_temporal_filter vs temporal_filter_ref, noc {noc}", ["out", "support"])
        at_offsets(gpu, want, f"tfilter_level, noc {noc}", call)


@by_case
def test_trajfilter_level(gpu, g, family):
    ufw, urev, _, _ = materialised(gpu, g, family)
    dfw, drev = level_devs(gpu, g, family)
    wo, ho = g[5], g[6]
    for noc in (1, 3):
        frames = frames_of(g, noc)
        df = gpu.Dev(frames)
        for fb in (1, 0):
            def call(out_ptr, sup_ptr):
                launch("trajfilter_level", df.ptr, dfw.ptr, drev.ptr, out_ptr, sup_ptr, NPAIRS, *g, noc, WEIGHTS.ctypes.data, WEIGHTS.size,
                       TAU, fb, ALPHA, BETA)

            out, sup = Out(gpu, img_shape(NPAIRS + 1, wo, ho, noc)), Out(gpu, (NPAIRS + 1, ho, wo))
            call(out.ptr, sup.ptr)
            sync(gpu)
            got = out.get("trajfilter_level out"), sup.get("trajfilter_level support")
            want = gpu.trajectory_filter(frames, ufw, urev, WEIGHTS, tau=TAU, fb_check=fb, alpha=ALPHA, beta=BETA)
            what = f"noc {noc}, fb_check {fb}"
            assert_all_same(got, want, f"trajfilter_level vs ofdis_trajectory_filter, {what}", ["out", "support"])
            if with_definition(g, family):
                assert_all_same(want, trajectory_filter_ref(frames, ufw, urev, WEIGHTS, TAU, bool(fb), ALPHA, BETA),
                                f"ofdis_trajectory_filter vs trajectory_filter_ref, {what}", ["out", "support"])
            at_offsets(gpu, want, f"trajfilter_level, {what}", call)


# order -> (fit hook, compensate hook, frames fit, frames compensate, numpy fit, numpy compensate, work bytes)
def _camera(gpu, order):
    if order == 6:
        return ("gmotion_level", "gmotion_compensate_level", lambda f, m: gpu.global_motion(f, m, gmotion.GM_AFFINE, GM_ROUNDS, GM_THRESH),
                lambda f, a, m: gpu.motion_compensate(f, a, m, GM_THRESH),
                lambda f, m: gmotion.global_motion_ref(f, m, gmotion.GM_AFFINE, GM_ROUNDS, GM_THRESH),
                lambda f, a, m: gmotion.motion_compensate_ref(f, a, m, GM_THRESH),
                lambda w, h: hooks().ofdis_test_gmotion_work_bytes(NPAIRS, w, h))
    return ("projective_level", "projective_compensate_level", lambda f, m: gpu.projective_motion(f, m, GM_ROUNDS, GM_THRESH),
            lambda f, a, m: gpu.projective_compensate(f, a, m, GM_THRESH),
            lambda f, m: gmotion.projective_motion_ref(f, m, GM_ROUNDS, GM_THRESH),
            lambda f, a, m: gmotion.projective_compensate_ref(f, a, m, GM_THRESH),
            lambda w, h: gpu.lib().ofdis_projective_motion_work_bytes(NPAIRS, w, h))


@by_case
def test_camera_models_level(gpu, g, family):
    """gmotion_level / gmotion_compensate_level and their projective twins, under the forward mask (rev given) and without a
    mask (rev null): there the exact family's pair of t = +-4096 meets the validity bound exactly and is fitted"""
    ufw, _, mf, _ = materialised(gpu, g, family)
    dfw, drev = level_devs(gpu, g, family)
    wo, ho = g[5], g[6]
    for order in (6, 8):
        fit_hook, comp_hook, fit, comp, fit_ref, comp_ref, work_bytes = _camera(gpu, order)
        for rev_ptr, mask in ((drev.ptr, mf), (None, None)):
            what = f"{order} parameters, {'forward mask' if mask is not None else 'no mask'}"
            models, stats = Out(gpu, (NPAIRS, order), np.float64), Out(gpu, (NPAIRS, 3), np.int64)
            work = gpu.Dev(nbytes=max(8, work_bytes(wo, ho)))
            model_arg = (gmotion.GM_AFFINE,) if order == 6 else ()
            launch(fit_hook, dfw.ptr, rev_ptr, NPAIRS, *g, *model_arg, GM_ROUNDS, GM_THRESH, ALPHA, BETA, models.ptr, stats.ptr, work.ptr)
            sync(gpu)
            got = models.get("models"), stats.get("stats")
            want = fit(ufw, mask)
            assert_all_same(got, want, f"{fit_hook} vs the frames form, {what}", ["models", "stats"])
            if family == "exact" and mask is None:   # (on the frames form) every pixel of the pair at the bound is in the set
                assert want[1][2, 0] == wo * ho, want[1]
            dmod = gpu.Dev(want[0])

            def call(lab_ptr, res_ptr=None):
                res = Out(gpu, (NPAIRS, ho, wo, 2), _f32)
                launch(comp_hook, dfw.ptr, rev_ptr, dmod.ptr, NPAIRS, *g, GM_THRESH, ALPHA, BETA, res.ptr, lab_ptr)
                return res

            lab = Out(gpu, (NPAIRS, ho, wo))
            res = call(lab.ptr)
            sync(gpu)
            gotc = res.get("residual"), lab.get("label")
            wantc = comp(ufw, want[0], mask)
            assert_all_same(gotc, wantc, f"{comp_hook} vs the frames form, {what}", ["residual", "label"])
            if with_definition(g, family):
                ref = fit_ref(ufw, mask)
                assert_all_same(want, ref, f"the frames fit vs gmotion.py, {what}", ["models", "stats"])
                refc = comp_ref(ufw, ref[0], mask)
                assert_bits_or_nan(wantc[0], refc[0], f"the frames residual vs gmotion.py, {what}")
                assert_same_bytes(wantc[1], refc[1], f"the frames labels vs gmotion.py, {what}")
            at_offsets(gpu, [wantc[1]], f"{comp_hook} labels, {what}", call)


def _seeds(wo, ho):
    """the four corners, points on the last row and column, points outside (NaN and infinite among them), integer pixels and
    real positions inside; seed frames from -1 to NPAIRS + 1, the first dozen at frame 0"""
    rng = np.random.default_rng(100 * wo + ho)
    X, Y = wo - 1, ho - 1
    pts = [(0, 0), (X, 0), (0, Y), (X, Y), (0.5 * X, Y), (0.25 * X, Y), (X, 0.5 * Y), (X, 0.75 * Y),
           (-0.5, 0), (X + 0.25, 0), (0, Y + 0.5), (wo, ho), (np.nan, 0), (0, np.inf), (-1, -1)]
    real = np.stack([rng.uniform(0, X, 40), rng.uniform(0, Y, 40)], axis=1)
    seeds = np.concatenate([np.asarray(pts, np.float64), real, np.rint(real)]).astype(_f32)
    frame = rng.integers(-1, NPAIRS + 2, len(seeds)).astype(np.int32)
    frame[:12] = 0
    return np.ascontiguousarray(seeds), frame


@by_case
def test_track_level(gpu, g, family):
    ufw, urev, _, _ = materialised(gpu, g, family)
    dfw, drev = level_devs(gpu, g, family)
    wo, ho = g[5], g[6]
    seeds, frame = _seeds(wo, ho)
    ds, dsf = gpu.Dev(seeds), gpu.Dev(frame)
    n = len(seeds)
    for with_rev in (True, False):
        for max_steps in (0, 2):
            tracks, counts = Out(gpu, (NPAIRS + 1, n, 2), _f32), Out(gpu, (n,), np.int32)
            launch("track_level", dfw.ptr, drev.ptr if with_rev else None, NPAIRS, *g, ds.ptr, dsf.ptr, n, max_steps, ALPHA, BETA,
                   tracks.ptr, counts.ptr)
            sync(gpu)
            got = tracks.get("tracks"), counts.get("counts")
            r = urev if with_rev else None
            want = gpu.track_points(ufw, r, seeds, frame, max_steps, ALPHA, BETA)
            what = f"{'with' if with_rev else 'without'} the test, max_steps {max_steps}"
            assert_all_same(got, want, f"track_level vs ofdis_track_points, {what}", ["tracks", "counts"])
            if with_definition(g, family):
                assert_all_same(want, tracking.track_ref(ufw, r, seeds, frame, max_steps, ALPHA, BETA),
                                f"ofdis_track_points vs track_ref, {what}", ["tracks", "counts"])
    if family != "wild" and wo * ho >= 30:   # (on the frames form) some track takes a step, some seed never starts
        assert (want[1] > 1).any() and (want[1] == 0).any(), want[1]


STRIDE, WINDOW = 2, 1


# (ofdis_dense_tracks rejects a side below the stride: at 5x1 and 1x6 there is no frames form to hold the level form to)
@pytest.mark.parametrize("g,family", [c for c in CASES if min(c.values[0][5:7]) >= STRIDE])
def test_dense_tracks_level(gpu, g, family):
    wo, ho = g[5], g[6]
    ufw, urev, _, _ = materialised(gpu, g, family)
    dfw, drev = level_devs(gpu, g, family)
    ncx, ncy = gpu.dense_tracks_cells(wo, ho, STRIDE)
    max_tracks = NPAIRS * ncx * ncy
    wb = gpu.lib().ofdis_dense_tracks_work_bytes(NPAIRS, wo, ho, STRIDE)
    for noc in (1, 3):
        frames = frames_of(g, noc)
        T = _threshold(frames[0], STRIDE, WINDOW, 0.6)
        df = gpu.Dev(frames)
        for with_rev in (True, False):
            for max_len in (0, 2):
                lmax = min(max_len, NPAIRS) if max_len else NPAIRS
                outs = gpu._dense_outputs(lmax, max_tracks)
                work = gpu.Dev(nbytes=max(8, wb))
                launch("dense_tracks_level", df.ptr, dfw.ptr, drev.ptr if with_rev else None, NPAIRS, *g, noc, STRIDE, WINDOW, T, max_len,
                       ALPHA, BETA, max_tracks, *[o.ptr for o in outs], work.ptr)
                sync(gpu)
                got = gpu._dense_results(outs, lmax, max_tracks)
                r = urev if with_rev else None
                want = gpu.dense_tracks(frames, ufw, r, STRIDE, WINDOW, T, max_len, alpha=ALPHA, beta=BETA)
                what = f"noc {noc}, {'with' if with_rev else 'without'} the test, max_len {max_len}"
                assert_dense_equal(got, want, f"dense_tracks_level vs ofdis_dense_tracks, {what}")
                if with_definition(g, family):
                    ref = tracking.dense_tracks_ref(frames, ufw, r, STRIDE, WINDOW, T, max_len, alpha=ALPHA, beta=BETA)
                    assert_dense_equal(want, ref, f"ofdis_dense_tracks vs dense_tracks_ref, {what}")
        assert want[3][0] > 0   # (on the frames form) tracks exist


def _disparities(g, family):
    """one-channel level disparities [NPAIRS][sh][sw] of the forward and the mirror pass: the x components of the planted flows;
    for coherent and exact the mirror pass is the forward one mirrored, so that DR = -mir(Dm) agrees with U and code 0 dominates"""
    fw, rev = level_flows(g, family)
    fwd = np.ascontiguousarray(fw[..., 0])
    mir = np.ascontiguousarray(rev[..., 0] if family == "wild" else fwd[:, :, ::-1])
    return fwd, mir


@by_case
def test_stereo_lr_level(gpu, g, family):
    """upsample_lr (the fused form, where upsample_lr_fuses(wo) says so) and lr_materialise with the composition on its outputs
    (the form above that width), both against tests/stereo_lr_ref.py on up_ref; the column of the mirror pass is
    (wo - 1 - x) + left"""
    wo, ho = g[5], g[6]
    fwd, mir = _disparities(g, family)
    u_ref, dm_ref = up_ref1(fwd, g), up_ref1(mir, g)
    dfw, dmir = gpu.Dev(fwd), gpu.Dev(mir)
    u, dr = Out(gpu, (NPAIRS, ho, wo), _f32), Out(gpu, (NPAIRS, ho, wo), _f32)
    launch("lr_materialise", dfw.ptr, dmir.ptr, u.ptr, dr.ptr, NPAIRS, *g)
    sync(gpu)
    u, dr = u.get("lr_materialise U"), dr.get("lr_materialise DR")
    assert_bits_or_nan(u, u_ref, "lr_materialise, U")
    assert_bits_or_nan(dr, stereo_lr_ref.right_view(dm_ref), "lr_materialise, DR")
    ml, mr = gpu.lr_check(u, dr, ALPHA, BETA), gpu.lr_check(dr, u, ALPHA, BETA)
    assert upsample_lr_fuses(wo)
    for fill in (gpu.FILL_NONE, gpu.FILL_INVALIDATE, gpu.FILL_BACKGROUND):
        want = stereo_lr_ref.compose(u_ref, dm_ref, fill, ALPHA, BETA)
        outs = [Out(gpu, (NPAIRS, ho, wo), _f32), Out(gpu, (NPAIRS, ho, wo), _f32), Out(gpu, (NPAIRS, ho, wo)), Out(gpu, (NPAIRS, ho, wo))]
        launch("upsample_lr", dfw.ptr, dmir.ptr, *[o.ptr for o in outs], NPAIRS, *g, fill, ALPHA, BETA)
        sync(gpu)
        got = [o.get(f"upsample_lr output {k}, fill {fill}") for k, o in enumerate(outs)]
        names = ["left disparity", "right disparity", "left mask", "right mask"]
        for k in (0, 1):
            assert_bits_or_nan(got[k], want[k], f"upsample_lr vs stereo_lr_ref, fill {fill}, {names[k]}")
        for k in (2, 3):
            assert_same_bytes(got[k], want[k], f"upsample_lr vs stereo_lr_ref, fill {fill}, {names[k]}")
        # the composition on the materialised arrays, the product's frames forms: byte for byte
        composed = [gpu.disparity_fill(u, ml, fill), gpu.disparity_fill(dr, mr, fill), ml, mr]
        assert_all_same(got, composed, f"upsample_lr vs the composition, fill {fill}", names)
    if family == "exact":
        k = 1   # t = -3: consistent where x - 3 >= 0
        assert (want[2][k][:, 3:] == 0).all() and (want[2][k][:, :3] == 2).all()
