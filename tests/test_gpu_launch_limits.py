"""-m gpu: every launcher's second chunk and second grid-stride trip.

Two host-side constants decide how the post-processing kernels cover their work (of_dis_amd/csrc/ofdis_kernels.h): one launch of
a quad kernel has at most QUAD_MAX_BLOCKS = 2^22 workgroups and the launcher walks the frames in chunks (f0, n); the grid of a
grid-stride kernel has at most GRID_MAX_BLOCKS = 2^20 workgroups and the kernel loops.  At test sizes neither a second chunk nor
a second trip is ever reached in libofdis_hip.so.  The test library links the same units with the two limits as variables
(tests/launch_hooks.py), so here they are lowered until 27 frames take nine launches and 2035 pixels eight trips.

Expected bytes: where a public entry point takes the same arrays, that entry point of libofdis_hip.so on the same inputs -- one
launch at these sizes, held to the numpy model by the feature's own tests; for the level routes and the internal launchers the
same hook with the limits at the product's values, plus one anchor per level route against the product's batch call on a real
context.  Every comparison is byte equality; every output is pre-filled with 0xAB and has a guard behind it.  That a case
really takes the launches or trips it is named for is asserted on the geometry functions, never on the kernel under test."""
import ctypes as C

import numpy as np
import pytest

import seq_products
import test_gpu_gmotion as gm_tests
import test_gpu_stabilize as stab_tests
from launch_hooks import chunk_walk, hooks, launch, quad_grid, trips
from of_dis_amd import encoding
from of_dis_amd.gmotion import GM_AFFINE
from of_dis_amd.stabilize import BORDER_CONSTANT, BORDER_REPLICATE
from of_dis_amd.temporal import reach, trajectory_weights
from trajfilter_cases import coherent_case, random_case

pytestmark = pytest.mark.gpu
_f32 = np.float32
AB, GUARD = 0xAB, 512
NPAIRS = 26   # 27 frames
SHAPES = [(64, 48), (37, 11)]   # bpf 3 with 4-byte stores; bpf 1, odd width, byte stores
SHAPE_IDS = ["64x48", "37x11"]
CHUNKS = [3, 8, 16]
ALPHA, BETA = 0.01, 0.5
TIMES = np.array([0.5, 0.0, 1.0, 0.3], _f32)
WEIGHTS = trajectory_weights(2, 0.75)   # radius 2: a walk crosses two chunk boundaries when the chunks are 3 frames
TAU, WN = 24.0, 0.75


# ------------------------------------------------------------------ helpers
@pytest.fixture
def limits():
    """limits(quad, grid) lowers the test library's limits (0: the product's value); they return to 0 afterwards, also on failure"""
    L = hooks()
    yield lambda quad=0, grid=0: L.ofdis_test_set_launch_limits(quad, grid)
    L.ofdis_test_set_launch_limits(0, 0)


class Out:
    """a device array [frames][...] pre-filled with 0xAB with a guard of 0xAB behind it"""

    def __init__(self, gpu, shape, dtype=np.uint8):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.dev = gpu.Dev(np.full(self.nbytes + GUARD, AB, np.uint8))
        self.ptr = self.dev.ptr

    def get(self, what):
        """the array; nothing written past its end and no frame left unwritten"""
        raw = self.dev.get((self.nbytes + GUARD,), np.uint8)
        assert (raw[self.nbytes:] == AB).all(), f"{what}: written past the end of the array"
        unwritten = np.flatnonzero((raw[:self.nbytes].reshape(self.shape[0], -1) == AB).all(axis=1))
        assert unwritten.size == 0, f"{what}: frames {unwritten.tolist()} were left unwritten"
        return raw[:self.nbytes].view(self.dtype).reshape(self.shape)


def assert_same_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = (np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1) for a in (got, want))
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        frames = sorted(set(bad[:, 0].tolist()))
        raise AssertionError(f"{what}: {len(bad)} of {g.size} bytes differ, in frames {frames}; first at frame {bad[0][0]}, "
                             f"byte {bad[0][1]}: {g[tuple(bad[0])]:#x} vs {w[tuple(bad[0])]:#x}")


def assert_all_same(got, want, what, names):
    for g, w, name in zip(got, want, names):
        assert_same_bytes(g, w, f"{what}, {name}")


def sync(gpu):
    gpu.check(gpu.lib().ofdis_sync(None))


_REFERENCES = {}


def reference(key, make):
    """the expected arrays of a case, computed once and shared by the cases that lower the limits differently"""
    if key not in _REFERENCES:
        ref = make()
        for a in ref:
            a.setflags(write=False)
        _REFERENCES[key] = ref
    return _REFERENCES[key]


def lower_quad_limit(limits, nitems, w, h, chunk):
    """QUAD_MAX_BLOCKS chosen so that `nitems` frames (or pairs) of w x h go in chunks of `chunk`; asserts on quad_grid that the
    walk is what the case is named for"""
    bpf, _ = quad_grid(nitems, w, h)
    assert bpf == -(-((w + 3) // 4 * h) // 256)
    limits(quad=chunk * bpf)
    _, walk = chunk_walk(nitems, w, h)
    sizes = [n for _, n, _ in walk]
    assert sizes == [min(chunk, nitems - f0) for f0 in range(0, nitems, chunk)] and len(sizes) >= 2, sizes
    assert all(blocks <= chunk * bpf for _, _, blocks in walk)
    if chunk == 3:    # nine launches, every one on the mapping for fewer than 8 frames
        assert len(sizes) == 9 and max(sizes) < 8
    elif chunk == 8:
        assert sizes[:3] == [8, 8, 8] and sizes[3] < 8
    else:             # a tail of at least 8 frames that is no multiple of 8
        assert sizes[0] == 16 and sizes[1] >= 8 and sizes[1] % 8 != 0
    return sizes


def wild_case(w, h, noc):
    """27 "smooth" frames (a ramp plus noise, so the intensity gates of the filters let neighbours in) with the "wild" flows of
    their 26 pairs (large, infinite, NaN and image-sized values mixed in), both from tests/trajfilter_cases.py"""
    return (random_case(NPAIRS, w, h, noc, "smooth")[0],) + random_case(NPAIRS, w, h, noc, "wild")[1:]


def img_shape(n, w, h, noc):
    return (n, h, w) + ((3,) if noc == 3 else ())


def _masks(n, w, h, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 3, (n, h, w), dtype=np.uint8) for _ in range(2)]


def up_geom(w, h):
    """a level flow a factor 2 below the padded size (a multiple of 4): 64x48 from 32x24; 37x11 from 20x6, cropped at left 1"""
    W, H = w + (-w) % 4, h + (-h) % 4
    return (W // 2, H // 2, 1, (W - w) // 2, (H - h) // 2, w, h)


def level_case(kind, w, h, noc):
    """27 frames of w x h and the level flows of their 26 pairs at up_geom(w, h), from tests/trajfilter_cases.py"""
    g = up_geom(w, h)
    frames = random_case(NPAIRS, w, h, noc, "smooth")[0]
    _, fw, rev = coherent_case(NPAIRS, g[0], g[1], 1) if kind == "coherent" else random_case(NPAIRS, g[0], g[1], 1, kind)
    return g, frames, fw, rev


# ------------------------------------------------------------------ 1. frames routes: the product's entry point is the reference
def _interp_hook(gpu, A, B, fw, rev, mf, mr, noc):
    n, h, w = fw.shape[:3]
    devs = [gpu.Dev(x) for x in (A, B, fw, rev, mf, mr)]
    out = Out(gpu, (n, TIMES.size) + img_shape(n, w, h, noc)[1:])
    launch("interp_frames", *[d.ptr for d in devs], out.ptr, n, w, h, noc, TIMES.ctypes.data, TIMES.size)
    sync(gpu)
    return (out.get("interp out"),)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", SHAPES, ids=SHAPE_IDS)
def test_interp_frames_in_chunks(gpu, limits, w, h, noc, chunk):
    frames, fw, rev = wild_case(w, h, noc)
    A, B = np.ascontiguousarray(frames[:-1]), np.ascontiguousarray(frames[1:])
    mf, mr = _masks(NPAIRS, w, h, 11)
    want = reference(("interp", w, h, noc), lambda: (gpu.interpolate(A, B, fw, rev, TIMES, mf, mr),))
    lower_quad_limit(limits, NPAIRS, w, h, chunk)
    assert_all_same(_interp_hook(gpu, A, B, fw, rev, mf, mr, noc), want, f"interp_frames, chunks of {chunk}", ["out"])


def _filter_outs(gpu, w, h, noc):
    return Out(gpu, img_shape(NPAIRS + 1, w, h, noc)), Out(gpu, (NPAIRS + 1, h, w))


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", SHAPES, ids=SHAPE_IDS)
def test_tfilter_frames_in_chunks(gpu, limits, w, h, noc, chunk):
    frames, fw, rev = wild_case(w, h, noc)
    mf, mr = _masks(NPAIRS, w, h, 12)
    want = reference(("tfilter", w, h, noc), lambda: gpu.temporal_filter(frames, fw, rev, mf, mr, wn=WN, tau=TAU))
    assert (want[1] == 3).any() and (want[1] == 0).any()   # (on the product's result) both neighbours used, and neither
    lower_quad_limit(limits, NPAIRS + 1, w, h, chunk)
    devs = [gpu.Dev(x) for x in (frames, fw, rev, mf, mr)]
    out, sup = _filter_outs(gpu, w, h, noc)
    launch("tfilter_frames", *[d.ptr for d in devs], out.ptr, sup.ptr, NPAIRS, w, h, noc, WN, TAU)
    sync(gpu)
    assert_all_same((out.get("out"), sup.get("support")), want, f"tfilter_frames, chunks of {chunk}", ["out", "support"])


def _walks_cross_boundaries(support, chunk):
    """(on a reference result) at every chunk boundary some pixel of the frame before it walks two frames forward and some pixel
    of the frame after it two frames back: with chunks of 3 that is across two boundaries for the frames next to one"""
    nb, nf = reach(support)
    for f0 in range(chunk, NPAIRS + 1 - 2, chunk):
        assert (nf[f0 - 1] == 2).any() and (nb[f0 + 1] == 2).any() and (nb[f0] == 2).any(), f0


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("kind", ["wild", "coherent"])
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", SHAPES, ids=SHAPE_IDS)
def test_trajfilter_frames_in_chunks(gpu, limits, w, h, noc, kind, chunk):
    frames, fw, rev = coherent_case(NPAIRS, w, h, noc) if kind == "coherent" else wild_case(w, h, noc)
    want = reference(("trajfilter", w, h, noc, kind),
                     lambda: gpu.trajectory_filter(frames, fw, rev, WEIGHTS, tau=TAU, fb_check=1, alpha=ALPHA, beta=BETA))
    if kind == "coherent":
        _walks_cross_boundaries(want[1], chunk)
    else:   # (on the product's result) walks that end at once and walks that do not
        assert (want[1] == 0).any() and (want[1] != 0).any()
    lower_quad_limit(limits, NPAIRS + 1, w, h, chunk)
    devs = [gpu.Dev(x) for x in (frames, fw, rev)]
    out, sup = _filter_outs(gpu, w, h, noc)
    launch("trajfilter_frames", *[d.ptr for d in devs], out.ptr, sup.ptr, NPAIRS, w, h, noc, WEIGHTS.ctypes.data, WEIGHTS.size, TAU,
           1, ALPHA, BETA)
    sync(gpu)
    assert_all_same((out.get("out"), sup.get("support")), want, f"trajfilter_frames {kind}, chunks of {chunk}", ["out", "support"])


GM_ROUNDS, GM_THRESH = 3, 1.0


def _gm_outs(gpu, w, h):
    return (Out(gpu, (NPAIRS, 6), np.float64), Out(gpu, (NPAIRS, 3), np.int64),
            gpu.Dev(nbytes=hooks().ofdis_test_gmotion_work_bytes(NPAIRS, w, h)))


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("kind", ["smooth", "wild"])
@pytest.mark.parametrize("w,h", SHAPES, ids=SHAPE_IDS)
def test_gmotion_frames_in_chunks(gpu, limits, w, h, kind, chunk):
    """the models as fp64 bit patterns and the stats after 3 rounds of the affine model, then the residual and labels under those
    models: the twelve sums are integers and every pair has slab records of its own, so the chunking cannot change a bit"""
    flow, mask = gm_tests._random_case(NPAIRS, w, h, kind)
    want = reference(("gmotion", w, h, kind), lambda: gpu.global_motion(flow, mask, GM_AFFINE, GM_ROUNDS, GM_THRESH))
    wantc = reference(("compensate", w, h, kind), lambda: gpu.motion_compensate(flow, want[0], mask, GM_THRESH))
    assert len({m.tobytes() for m in want[0]}) == NPAIRS   # (on the product's result) every pair has a model of its own ...
    if kind == "smooth":                                  # ... and the gate removes pixels in most pairs
        assert (want[1][:, 1] < want[1][:, 0]).sum() > NPAIRS // 2
    assert hooks().ofdis_test_gmotion_work_bytes(NPAIRS, w, h) == gpu.lib().ofdis_global_motion_work_bytes(NPAIRS, w, h)
    lower_quad_limit(limits, NPAIRS, w, h, chunk)
    df, dm = gpu.Dev(flow), gpu.Dev(mask)
    models, stats, work = _gm_outs(gpu, w, h)
    launch("gmotion_frames", df.ptr, dm.ptr, NPAIRS, w, h, GM_AFFINE, GM_ROUNDS, GM_THRESH, models.ptr, stats.ptr, work.ptr)
    sync(gpu)
    assert_all_same((models.get("models"), stats.get("stats")), want, f"gmotion_frames, chunks of {chunk}", ["models", "stats"])
    dmod = gpu.Dev(want[0])
    res, lab = Out(gpu, (NPAIRS, h, w, 2), _f32), Out(gpu, (NPAIRS, h, w))
    launch("gmotion_compensate_frames", df.ptr, dm.ptr, dmod.ptr, NPAIRS, w, h, GM_THRESH, res.ptr, lab.ptr)
    sync(gpu)
    assert_all_same((res.get("residual"), lab.get("label")), wantc, f"gmotion_compensate_frames, chunks of {chunk}",
                    ["residual", "label"])


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("border", [BORDER_CONSTANT, BORDER_REPLICATE], ids=["constant", "replicate"])
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", SHAPES, ids=SHAPE_IDS)
def test_warp_frames_in_chunks(gpu, limits, w, h, noc, border, chunk):
    """the eleven warps of tests/test_gpu_stabilize.py (zero, translations, a rotation, NaN, all outside, infinite, random affines)
    repeated over 27 random frames, so every chunk has some of each"""
    nframes = NPAIRS + 1
    frames = random_case(NPAIRS, w, h, noc, "wild")[0]
    warps = np.ascontiguousarray(np.resize(stab_tests._warp_case(w, h, noc)[1], (nframes, 6)))
    want = reference(("warp", w, h, noc, border), lambda: gpu.warp_frames(frames, warps, border))
    lower_quad_limit(limits, nframes, w, h, chunk)
    df, dw = gpu.Dev(frames), gpu.Dev(warps)
    out, ins = Out(gpu, img_shape(nframes, w, h, noc)), Out(gpu, (nframes, h, w))
    launch("warp_frames", df.ptr, dw.ptr, out.ptr, ins.ptr, nframes, w, h, noc, int(border == BORDER_REPLICATE))
    sync(gpu)
    # (an all-outside frame with a constant border is all zero, never all 0xAB)
    assert_all_same((out.get("out"), ins.get("inside")), want, f"warp_frames, chunks of {chunk}", ["out", "inside"])


# ------------------------------------------------------------------ 2. level routes: the same hook at the product's limits
def _interp_bidir(gpu, g, A, B, fw, rev, noc):
    n = fw.shape[0]
    devs = [gpu.Dev(x) for x in (A, B, fw, rev)]
    out = Out(gpu, (n, TIMES.size) + img_shape(n, g[5], g[6], noc)[1:])
    launch("interp_bidir", *[d.ptr for d in devs], out.ptr, n, *g, noc, TIMES.ctypes.data, TIMES.size, ALPHA, BETA)
    sync(gpu)
    return (out.get("interp_bidir out"),)


def _tfilter_level(gpu, g, frames, fw, rev, noc):
    n = fw.shape[0]
    devs = [gpu.Dev(x) for x in (frames, fw, rev)]
    out, sup = Out(gpu, img_shape(n + 1, g[5], g[6], noc)), Out(gpu, (n + 1, g[6], g[5]))
    launch("tfilter_level", *[d.ptr for d in devs], out.ptr, sup.ptr, n, *g, noc, WN, TAU, ALPHA, BETA)
    sync(gpu)
    return out.get("tfilter_level out"), sup.get("tfilter_level support")


def _trajfilter_level(gpu, g, frames, fw, rev, noc):
    n = fw.shape[0]
    devs = [gpu.Dev(x) for x in (frames, fw, rev)]
    out, sup = Out(gpu, img_shape(n + 1, g[5], g[6], noc)), Out(gpu, (n + 1, g[6], g[5]))
    launch("trajfilter_level", *[d.ptr for d in devs], out.ptr, sup.ptr, n, *g, noc, WEIGHTS.ctypes.data, WEIGHTS.size, TAU, 1, ALPHA,
           BETA)
    sync(gpu)
    return out.get("trajfilter_level out"), sup.get("trajfilter_level support")


def _gmotion_level(gpu, g, fw, rev):
    n = fw.shape[0]
    dfw, drev = gpu.Dev(fw), gpu.Dev(rev)
    models, stats = Out(gpu, (n, 6), np.float64), Out(gpu, (n, 3), np.int64)
    work = gpu.Dev(nbytes=hooks().ofdis_test_gmotion_work_bytes(n, g[5], g[6]))
    launch("gmotion_level", dfw.ptr, drev.ptr, n, *g, GM_AFFINE, GM_ROUNDS, GM_THRESH, ALPHA, BETA, models.ptr, stats.ptr, work.ptr)
    sync(gpu)
    return models.get("gmotion_level models"), stats.get("gmotion_level stats")


def _compensate_level(gpu, g, fw, rev, models):
    n = fw.shape[0]
    dfw, drev, dmod = gpu.Dev(fw), gpu.Dev(rev), gpu.Dev(models)
    res, lab = Out(gpu, (n, g[6], g[5], 2), _f32), Out(gpu, (n, g[6], g[5]))
    launch("gmotion_compensate_level", dfw.ptr, drev.ptr, dmod.ptr, n, *g, GM_THRESH, ALPHA, BETA, res.ptr, lab.ptr)
    sync(gpu)
    return res.get("compensate_level residual"), lab.get("compensate_level label")


def _level_routes(gpu, g, frames, fw, rev, noc):
    """every level route on one clip: {route: its output arrays}; frame pairs for the interpolation are (k, k + 1)"""
    A, B = np.ascontiguousarray(frames[:-1]), np.ascontiguousarray(frames[1:])
    fit = _gmotion_level(gpu, g, fw, rev)
    return {"interp_bidir": _interp_bidir(gpu, g, A, B, fw, rev, noc), "tfilter_level": _tfilter_level(gpu, g, frames, fw, rev, noc),
            "trajfilter_level": _trajfilter_level(gpu, g, frames, fw, rev, noc), "gmotion_level": fit,
            "gmotion_compensate_level": _compensate_level(gpu, g, fw, rev, fit[0])}


def _flat_reference(key, make):
    """reference() for a dict of tuples"""
    if key not in _REFERENCES:
        _REFERENCES[key] = make()
        for arrays in _REFERENCES[key].values():
            for a in arrays:
                a.setflags(write=False)
    return _REFERENCES[key]


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("kind", ["wild", "coherent"])
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", SHAPES, ids=SHAPE_IDS)
def test_level_routes_in_chunks(gpu, limits, w, h, noc, kind, chunk):
    """interp_bidir, tfilter_level, trajfilter_level, gmotion_level and gmotion_compensate_level from level flows a factor 2 below
    full resolution: in chunks, the bytes of one launch"""
    g, frames, fw, rev = level_case(kind, w, h, noc)
    limits(0, 0)
    assert len(chunk_walk(NPAIRS + 1, w, h)[1]) == 1
    want = _flat_reference(("level", w, h, noc, kind), lambda: _level_routes(gpu, g, frames, fw, rev, noc))
    if kind == "coherent":   # (on the one-launch result) walks of two steps at the chunk boundaries, some models fitted
        _walks_cross_boundaries(want["trajfilter_level"][1], chunk)
        assert (want["gmotion_level"][1][:, 0] > 0).all()
    lower_quad_limit(limits, NPAIRS, w, h, chunk)
    lower_quad_limit(limits, NPAIRS + 1, w, h, chunk)
    got = _level_routes(gpu, g, frames, fw, rev, noc)
    for route in want:
        assert_all_same(got[route], want[route], f"{route} {kind}, chunks of {chunk}", ["first output", "second output"])


# ------------------------------------------------------------------ 3. anchors: the level routes against the product's batch calls
@pytest.fixture(scope="module")
def seq_context(gpu):
    """a real SEQUENCE | REVERSE context over 27 gray frames of 64x48 at operating point 2, run: what its batch calls return, and
    its level flows and UpGeom as ofdis_products.hip makes it (finish_begin)"""
    w, h = SHAPES[0]
    clip = seq_products.smooth_clip(w, h, 1, NPAIRS + 1)
    b, devs = seq_products.run_context(gpu, clip, "seq_rev")
    try:
        p = b.p
        fw, rev = b.level_flow(p.sc_l), b.level_flow_reverse(p.sc_l)
        lw, lh = p.level_size(p.sc_l)
        g = (lw, lh, p.sc_l, (p.width - w) // 2, (p.height - h) // 2, w, h)
        fit = b.global_motion(w, h, GM_AFFINE, GM_ROUNDS, GM_THRESH, fb_check=True, alpha=ALPHA, beta=BETA)
        want = {"tfilter_level": b.temporal_filter(devs[0].ptr, w, h, wn=WN, tau=TAU, alpha=ALPHA, beta=BETA, support=True),
                "trajfilter_level": b.trajectory_filter(devs[0].ptr, w, h, WEIGHTS, tau=TAU, fb_check=True, alpha=ALPHA, beta=BETA,
                                                        support=True),
                "gmotion_level": fit,
                "gmotion_compensate_level": b.motion_compensate(fit[0], w, h, GM_THRESH, fb_check=True, alpha=ALPHA, beta=BETA)}
    finally:
        b.close()
    assert fw.shape == (NPAIRS, lh, lw, 2) and rev.shape == fw.shape
    return g, clip, fw, rev, want


@pytest.fixture(scope="module")
def reverse_context(gpu):
    """the same clip's pairs in a plain REVERSE context: ofdis_batch_interpolate and the level flows it reads"""
    w, h = SHAPES[0]
    clip = seq_products.smooth_clip(w, h, 1, NPAIRS + 1)
    b, devs = seq_products.run_context(gpu, clip, "reverse")
    try:
        p = b.p
        fw, rev = b.level_flow(p.sc_l), b.level_flow_reverse(p.sc_l)
        lw, lh = p.level_size(p.sc_l)
        g = (lw, lh, p.sc_l, (p.width - w) // 2, (p.height - h) // 2, w, h)
        want = b.interpolate(devs[0].ptr, devs[1].ptr, w, h, TIMES, alpha=ALPHA, beta=BETA)
    finally:
        b.close()
    return g, clip, fw, rev, want


@pytest.mark.parametrize("chunk", CHUNKS)
def test_level_routes_in_chunks_against_the_batch_calls(gpu, limits, seq_context, chunk):
    g, clip, fw, rev, want = seq_context
    w, h = SHAPES[0]
    lower_quad_limit(limits, NPAIRS, w, h, chunk)
    lower_quad_limit(limits, NPAIRS + 1, w, h, chunk)
    fit = _gmotion_level(gpu, g, fw, rev)
    got = {"tfilter_level": _tfilter_level(gpu, g, clip, fw, rev, 1), "trajfilter_level": _trajfilter_level(gpu, g, clip, fw, rev, 1),
           "gmotion_level": fit, "gmotion_compensate_level": _compensate_level(gpu, g, fw, rev, want["gmotion_level"][0])}
    for route in want:
        assert_all_same(got[route], want[route], f"{route} vs the context's batch call, chunks of {chunk}", ["first output", "second output"])


@pytest.mark.parametrize("chunk", CHUNKS)
def test_interp_bidir_in_chunks_against_the_batch_call(gpu, limits, reverse_context, chunk):
    g, clip, fw, rev, want = reverse_context
    lower_quad_limit(limits, NPAIRS, *SHAPES[0], chunk)
    got = _interp_bidir(gpu, g, np.ascontiguousarray(clip[:-1]), np.ascontiguousarray(clip[1:]), fw, rev, 1)
    assert_same_bytes(got[0], want, f"interp_bidir vs ofdis_batch_interpolate, chunks of {chunk}")


# ------------------------------------------------------------------ 4. grid-stride kernels
GRIDS = [1, 3]
ENCODINGS = {"f32": encoding.F32, "f16": encoding.F16, "u16": encoding.KITTI_FLOW, "u8": encoding.u8_bound(20)}


def _encode_values(n):
    rng = np.random.default_rng(n)
    v = (rng.standard_normal(n) * 12).astype(_f32)
    v[rng.integers(0, n, n // 50)] *= 1e-6   # (half's subnormal range)
    for x in (np.nan, np.inf, -np.inf, -0.0, 600.0, -600.0):
        v[rng.integers(0, n, n // 100)] = x
    return v


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n,offset", [(10007, 0), (10007, 1), (16 * 768 + 5, 0)], ids=["10007", "10007-off-4-bytes", "16x768+5"])
@pytest.mark.parametrize("name", sorted(ENCODINGS))
def test_encode_in_trips(gpu, limits, name, n, offset, grid):
    """aligned (16-byte stores and a scalar tail), from a source 4 bytes off (all scalar), and a length whose vector part ends
    exactly on a trip of 768 lanes for one-byte elements"""
    enc = ENCODINGS[name]
    es, per16 = enc.dtype.itemsize, 16 // enc.dtype.itemsize
    v = _encode_values(n)
    src = gpu.Dev(np.concatenate([np.zeros(offset, _f32), v]))

    def run(call):
        dst = gpu.Dev(np.full(n * es + GUARD, AB, np.uint8))
        call(src.ptr + 4 * offset, dst.ptr)
        sync(gpu)
        raw = dst.get((n * es + GUARD,), np.uint8)
        assert (raw[n * es:] == AB).all(), "written past the end"
        return raw[:n * es]

    want = reference(("encode", name, n, offset),
                     lambda: (run(lambda s, d: gpu.check(gpu.lib().ofdis_encode(s, d, n, C.byref(enc), None))),))[0]
    limits(grid=grid)
    nvec = 0 if offset else n // per16
    work = max(nvec, n - nvec * per16)
    assert trips(work) == -(-work // (256 * min(grid, -(-work // 256))))
    assert trips(work) >= 2 or grid == 3, (work, grid)
    if (n, name, grid) == (16 * 768 + 5, "u8", 3):
        assert nvec == 768 and trips(work) == 1 and n - nvec * per16 == 5
    got = run(lambda s, d: launch("encode", s, d, n, enc.type, enc.scale, enc.offset))
    assert np.array_equal(got, want), (name, n, offset, grid, np.flatnonzero(got != want)[:8] // es)


def _flows_5(w, h):
    _, fw, rev = random_case(5, w, h, 1, "wild")
    return fw, rev


def _disp(rng, shape, w):
    """disparities as _random_disp of tests/test_gpu_stereo_lr.py makes them"""
    d = (rng.standard_normal(shape) * (w / 6.0 + 1.0)).astype(_f32)
    flat = d.reshape(-1)
    k = max(1, flat.size // 50)
    for v in (np.nan, np.inf, -np.inf, 3.0 * w, -3.0 * w, 0.0, -0.0):
        flat[rng.integers(0, flat.size, k)] = v
    return d


@pytest.mark.parametrize("grid", GRIDS)
def test_fb_check_in_trips(gpu, limits, grid):
    """5 frames of 37x11: a trip of 256 or 768 pixels straddles frame boundaries"""
    w, h, n = 37, 11, 5
    fw, rev = _flows_5(w, h)
    want = reference(("fb_check",), lambda: (gpu.fb_check(fw, rev, ALPHA, BETA),))[0]
    assert len(np.unique(want)) == 3
    limits(grid=grid)
    assert trips(n * w * h) >= 2 and 256 * grid % (w * h) != 0
    df, do, mask = gpu.Dev(fw), gpu.Dev(rev), Out(gpu, (n, h, w))
    launch("fb_check", df.ptr, do.ptr, mask.ptr, n, w, h, ALPHA, BETA)
    sync(gpu)
    assert_same_bytes(mask.get("mask"), want, f"fb_check, grid of {grid}")


@pytest.mark.parametrize("grid", GRIDS)
def test_lr_check_and_disparity_fill_in_trips(gpu, limits, grid):
    w, h, n = 37, 11, 5
    rng = np.random.default_rng(371105)
    d, o = _disp(rng, (n, h, w), w), _disp(rng, (n, h, w), w)
    d[:, 0], o[:, 0] = -1.0, 1.0   # (a row that is consistent from x = 1: the three codes all occur)
    want = reference(("lr_check",), lambda: (gpu.lr_check(d, o, ALPHA, BETA),))[0]
    assert len(np.unique(want)) == 3
    fills = {mode: reference(("fill", mode), lambda: (gpu.disparity_fill(d, want, mode),))[0] for mode in (gpu.FILL_NONE, gpu.FILL_INVALIDATE)}
    limits(grid=grid)
    assert trips(n * w * h) >= 2
    dd, do, mask = gpu.Dev(d), gpu.Dev(o), Out(gpu, (n, h, w))
    launch("lr_check", dd.ptr, do.ptr, mask.ptr, n, w, h, ALPHA, BETA)
    sync(gpu)
    assert_same_bytes(mask.get("mask"), want, f"lr_check, grid of {grid}")
    dm = gpu.Dev(want)
    for mode, filled in fills.items():   # NONE: out different from disp (a copy); INVALIDATE
        out = Out(gpu, (n, h, w), _f32)
        launch("disparity_fill", dd.ptr, dm.ptr, out.ptr, n, w, h, mode)
        sync(gpu)
        assert_same_bytes(out.get("filled"), filled, f"disparity_fill mode {mode}, grid of {grid}")
    assert np.isinf(fills[gpu.FILL_INVALIDATE]).sum() > np.isinf(d).sum()


@pytest.mark.parametrize("grid", GRIDS)
def test_mirror_u8_in_trips(gpu, limits, grid):
    w, h, n, noc = 37, 11, 3, 3
    frames = np.random.default_rng(37113).integers(0, 256, (n, h, w, noc), dtype=np.uint8)

    def run():
        src, dst = gpu.Dev(frames), Out(gpu, frames.shape)
        launch("mirror_u8", src.ptr, dst.ptr, n, w, h, noc)
        sync(gpu)
        return dst.get("mirrored")

    limits(0, 0)
    want = reference(("mirror",), lambda: (run(),))[0]
    assert np.array_equal(want, frames[:, :, ::-1])   # (the one-launch result is the definition)
    limits(grid=grid)
    assert trips(frames.size) >= 2
    assert_same_bytes(run(), want, f"mirror_u8, grid of {grid}")


# (noc, l, sc_f) of an operating point: the level arguments ofdis_batch_build_pyramids_u8 passes are (wo, ho, the size padded to
# 2^sc_f, noc, l = sc_l).  Operating points 1 and 2 have sc_l = sc_f - 2: l = 2, 3, 4 are what 512, 1024 and 2048 pixel wide gray
# frames get (pyr_base16_kernel<4 | 8 | 16>); RGB and l < 2 take pyr_base_kernel
PYR_LEVELS = [pytest.param(1, 2, 4, id="gray-l2-base16<4>"), pytest.param(1, 3, 5, id="gray-l3-base16<8>"),
              pytest.param(1, 4, 6, id="gray-l4-base16<16>"), pytest.param(3, 1, 3, id="rgb-l1-base"),
              pytest.param(1, 0, 1, id="gray-l0-base")]


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nframes", [3, 64])
@pytest.mark.parametrize("noc,l,sc_f", PYR_LEVELS)
def test_pyr_base_in_trips(gpu, limits, noc, l, sc_f, nframes, grid):
    """3 frames of 64x48, and 64 of them: a lane of pyr_base16_kernel<16> makes 16 outputs, so 3 frames are 48 lanes, and only the
    longer clip takes a second trip of 256 lanes there"""
    wo, ho = SHAPES[0]
    W, H = wo + (-wo) % (1 << sc_f), ho + (-ho) % (1 << sc_f)
    frames = np.random.default_rng(100 * l + noc).integers(0, 256, img_shape(nframes, wo, ho, noc), dtype=np.uint8)
    shape = (nframes, H >> l, W >> l) + ((3,) if noc == 3 else ())

    def run():
        src, dst = gpu.Dev(frames), Out(gpu, shape, _f32)
        launch("pyr_base", src.ptr, dst.ptr, nframes, wo, ho, W, H, noc, l, wo * noc, wo * noc * ho)
        sync(gpu)
        return dst.get("level image")

    limits(0, 0)
    want = reference(("pyr_base", noc, l, nframes), lambda: (run(),))[0]
    if W == wo and H == ho:   # (the one-launch result is the definition: block means, exact in fp32)
        blocks = frames.reshape(nframes, H >> l, 1 << l, W >> l, 1 << l, noc).astype(np.float64).mean(axis=(2, 4))
        assert np.array_equal(want.reshape(blocks.shape), blocks.astype(_f32))
    limits(grid=grid)
    streaming = noc == 1 and l in (2, 3, 4)
    work = nframes * (H >> l) * (W // 16) if streaming else int(np.prod(shape))
    assert trips(work) >= 2 or (nframes == 3 and streaming), (work, grid)
    assert_same_bytes(run(), want, f"pyr_base noc {noc} level {l}, {nframes} frames, grid of {grid}")


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("noc", [1, 3])
def test_pyr_down_in_trips(gpu, limits, noc, grid):
    w, h, n = 64, 48, 3
    src = np.random.default_rng(640 + noc).integers(0, 1021, img_shape(n, w, h, noc)).astype(_f32) * _f32(0.25)

    def run():
        ds, dst = gpu.Dev(src), Out(gpu, img_shape(n, w // 2, h // 2, noc), _f32)
        launch("pyr_down", ds.ptr, dst.ptr, n, w, h, noc)
        sync(gpu)
        return dst.get("next level")

    limits(0, 0)
    want = reference(("pyr_down", noc), lambda: (run(),))[0]
    s4 = src.reshape(n, h // 2, 2, w // 2, 2, noc).astype(np.float64).mean(axis=(2, 4))   # (quarters of 10-bit integers: exact)
    assert np.array_equal(want.reshape(s4.shape), s4.astype(_f32))
    limits(grid=grid)
    assert trips(want.size) >= 2
    assert_same_bytes(run(), want, f"pyr_down noc {noc}, grid of {grid}")


# ------------------------------------------------------------------ 5. the limits belong to the test library alone
def test_the_product_library_ignores_the_test_librarys_limits(gpu, limits):
    """libofdis_hip.so and libofdis_testhooks.so are separate objects: the product has the limits compiled in as constants, so its
    results while the test library's limits are at 1 workgroup are its results before"""
    w, h = SHAPES[1]
    frames, fw, rev = coherent_case(NPAIRS, w, h, 1)

    def product():
        return (gpu.trajectory_filter(frames, fw, rev, WEIGHTS, tau=TAU) + (gpu.fb_check(fw, rev),)
                + (gpu.encode(fw, ENCODINGS["f16"]).view(np.uint16),))

    before = product()
    limits(quad=1, grid=1)
    assert quad_grid(NPAIRS + 1, w, h) == (1, 1) and trips(fw.size) > 2
    during = product()
    limits(0, 0)
    assert quad_grid(NPAIRS + 1, w, h) == (1, NPAIRS + 1)
    assert_all_same(during, before, "the product under lowered test limits", ["out", "support", "fb mask", "f16"])
