"""Stereo-depth mode (the reference's run_DE_* binaries, compile-time SELECTMODE=2; ofdis_params.selectmode = 2):
one horizontal displacement per patch / pixel, constrained to <= 0 for the left camera.  The checker is the reference
itself compiled in that mode (oracle/_ref/libofdis_ref_de_*.so); the C restatement covers optical flow only."""
import numpy as np
import pytest

import oracle
from common import assert_bits_equal, rand_planes, synth_case

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["per-stage kernels", "fused stereo kernel"])
def stereo_tv(gpu, request):
    """Every test of this file twice: with the refinement on de_system + de_sor per fixed-point iteration (what exact-contract
    contexts of fewer than 256 frames run by default) and with levels of at most 64 rows forced onto de_fused_kernel (all
    iterations in one launch; ofdis_tuning.fused_rgb_min = 1)."""
    old = gpu.set_tuning(fused_rgb_min=1 if request.param.startswith("fused") else (1 << 30))
    yield request.param
    gpu.restore_tuning(old)


def _case(w, h, seed, noc, opp, tv):
    p, pa, pb, _, _ = synth_case(w, h, seed, noc, opp, tv)
    p = p.copy(selectmode=2)
    # The synthetic pair moves by about (+6, -3) px, so matching the SECOND image against the first sees a negative
    # horizontal displacement, which is what the left camera's constraint (<= 0) admits.  The vertical component
    # only makes the 1-D search work harder -- parity, not accuracy, is what is tested.
    return p, pb, pa


def _ref(noc):
    kind = "de_int" if noc == 1 else "de_rgb"
    R = oracle.need_ref(kind, True)
    if R is None:
        pytest.skip("comparison against the compiled reference skipped: neither /root/reference nor oracle/_ref exists here")
    return R


@pytest.mark.parametrize("noc,opp", [(1, 2), (3, 3), (1, 3), (3, 2)])
def test_stereo_patchgrid_levels(gpu, noc, opp):
    p, pa, pb = _case(640, 480, 90, noc, opp, 0)
    R = _ref(noc)
    prev = None
    for l in range(p.sc_f, p.sc_l - 1, -1):
        rp, rflow = R.patchgrid_level(p, l, pa[0][l], pa[1][l], pa[2][l], pb[0][l], prev)
        gp, gflow = gpu.patchgrid_level(p, l, pa[0][l][None], pa[1][l][None], pa[2][l][None], pb[0][l][None],
                                        prev[None] if prev is not None else None)
        assert rflow.shape[-1] == 1
        assert (rp[:, 0] <= 0).all() and (rp[:, 1] == 0).all()     # left camera: disparity <= 0 (patch.cpp:190)
        assert_bits_equal(gp[0], rp, f"stereo patch displacements level {l}")
        assert_bits_equal(gflow[0], rflow, f"stereo dense displacement level {l}")
        prev = rflow


@pytest.mark.parametrize("noc,size,opp,solverit", [(1, (640, 480), 2, 0), (1, (1024, 436), 2, 0), (3, (320, 240), 3, 0),
                                                   (1, (333, 251), 3, 0), (1, (600, 300), 3, 5), (1, (1242, 375), 2, 5),
                                                   (1, (640, 480), 2, 1), (1, (520, 1100), 3, 2)])
def test_stereo_varref_levels(gpu, noc, size, opp, solverit):
    """Levels of at most 64 rows (several frames per wavefront), taller ones (one workgroup per frame, the wavefronts
    in lock step: operating point 3 ends at half resolution), and solver sweep counts on either side of what one pass
    pipelines (4, or 3 above 64 rows)."""
    p, pa, pb = _case(size[0], size[1], 91, noc, opp, 1)
    if solverit:
        p = p.copy(tv_solverit=solverit)
    R = _ref(noc)
    rng = np.random.default_rng(4)
    for l in range(p.sc_f, p.sc_l - 1, -1):
        w, h = p.level_size(l)
        flow = -np.abs(rand_planes(rng, h, w, 1, scale=1.5))
        flow[::7, ::5] = 0.3                                        # some positive values: clamped by the update
        ref = R.varref_level(p, l, pa[0][l], pb[0][l], flow)
        got = gpu.varref_level(p, l, pa[0][l][None], pb[0][l][None], flow[None])
        assert_bits_equal(got[0], ref, f"stereo varref level {l}")


@pytest.mark.parametrize("size,noc,opp,tv", [((1024, 436), 1, 2, 1), ((640, 480), 1, 2, 0), ((333, 251), 1, 1, 1),
                                             ((320, 240), 3, 3, 1), ((333, 251), 1, 3, 1), ((200, 160), 1, 4, 0), ((320, 240), 3, 2, 1)])
def test_stereo_flow_bit_exact(gpu, size, noc, opp, tv):
    p, pa, pb = _case(size[0], size[1], 92, noc, opp, tv)
    R = _ref(noc)
    ref = R.flow(p, pa[0], pa[1], pa[2], pb[0])
    assert ref.shape[-1] == 1 and (ref <= 0).all()
    got = gpu.flow(p, pa[0], pa[1], pa[2], pb[0])
    assert_bits_equal(got, ref, "stereo displacement vs reference sources (SELECTMODE=2)")
    S = oracle.need_ref("de_int", False) if noc == 1 else None
    if S is not None:
        seq = S.flow(p, pa[0], pa[1], pa[2], pb[0])
        assert np.abs(seq - got).mean() * (1 << p.sc_l) < 1e-3      # any summation order lands within the tolerance
    b = gpu.Batch(p, 3)
    for k in range(3):
        b.upload(k, pa[0], pa[1], pa[2], pb[0])
    b.run()
    out = b.download_all()
    full = b.upsample(size[0], size[1])
    b.close()
    assert out.shape[-1] == 1 and full.shape == (3, size[1], size[0], 1)
    for k in range(3):
        assert_bits_equal(out[k], ref, f"batch frame {k}")


@pytest.mark.parametrize("size,noc,opp,tv", [((640, 480), 1, 2, 1), ((333, 251), 1, 1, 0), ((320, 240), 3, 3, 1)])
def test_stereo_forward_backward(gpu, size, noc, opp, tv):
    """usefbcon in stereo mode: the backward grid is the right camera (displacement >= 0, patch.cpp:191-192,
    refine_variational.cpp:308-315), merged one-channel splats (patchgrid.cpp:366-371)."""
    p, pa, pb = _case(size[0], size[1], 93, noc, opp, tv)
    p = p.copy(usefbcon=1)
    R = _ref(noc)
    ref = R.flow(p, pa[0], pa[1], pa[2], pb[0], pyr_b_dx=pb[1], pyr_b_dy=pb[2])
    plain = R.flow(p.copy(usefbcon=0), pa[0], pa[1], pa[2], pb[0])
    assert not np.array_equal(ref, plain)
    got = gpu.flow(p, pa[0], pa[1], pa[2], pb[0], pyr_b_dx=pb[1], pyr_b_dy=pb[2])
    assert_bits_equal(got, ref, "stereo + usefbcon vs reference sources")


@pytest.mark.parametrize("nsub", [2, 4])
def test_stereo_forward_backward_pipelined(gpu, nsub):
    """usefbcon in stereo mode on frame views (ofdis_batch_set_pipeline): the one configuration whose backward flow arrays
    hold ONE channel per pixel, so a sub-batch's share of them starts at w * h floats per frame, not 2 * w * h.  Every frame of
    the pipelined context -- different pairs, a ragged split -- has the bits of the un-pipelined context, and of the reference
    sources where they are present."""
    cases = [_case(640, 480, 94 + k, 1, 2, 1) for k in range(3)]
    p = cases[0][0].copy(usefbcon=1)
    order = [0, 1, 2, 2, 1, 0, 1]
    outs = []
    for pipeline in (0, nsub):
        b = gpu.Batch(p, len(order))
        for slot, k in enumerate(order):
            _, pa, pb = cases[k]
            b.upload(slot, pa[0], pa[1], pa[2], pb[0])
            b.upload_b_gradients(slot, pb[1], pb[2])
        b.set_pipeline(pipeline)
        b.run()
        b.run()                                  # two passes in flight before anything joins
        outs.append(b.download_all())
        b.close()
    R = oracle.need_ref("de_int", True)
    for slot, k in enumerate(order):
        assert_bits_equal(outs[1][slot], outs[0][slot], f"pipelined({nsub}) slot {slot} (pair {k}) vs the un-pipelined context")
        if R is not None and slot < 3:
            _, pa, pb = cases[k]
            ref = R.flow(p, pa[0], pa[1], pa[2], pb[0], pyr_b_dx=pb[1], pyr_b_dy=pb[2])
            assert_bits_equal(outs[0][slot], ref, f"slot {slot} (pair {k}) vs reference sources")


# ------------------------------------------------------------------ levels of free size, several DISTINCT frames per call
# ad-hoc campaigns: OFDIS_TEST_SEED_OFFSET=<n> shifts every seeded random draw below
_SEED_OFFSET = int(__import__("os").environ.get("OFDIS_TEST_SEED_OFFSET", "0"))


def _free_level(w, h, noc, seed, **over):
    """Parameters of a one-level stereo pyramid of free size (test_gpu_kernels.py::test_random_varref_levels' construction)
    and three synthetic pairs of that size, second image as the left camera: (p, [(pyr_left, pyr_right)] * 3)."""
    import gen_synth
    from of_dis_amd.params import oppoint
    P = over.get("p_samp_s", 4)
    p = oppoint(2, w, h, noc=noc).copy(sc_f=0, sc_l=0, imgpadding=P, selectmode=2, **dict(over, p_samp_s=P))
    p.width, p.height = w, h
    O = oracle.c_oracle()
    pairs = []
    for k in range(3):
        ia, ib, _ = gen_synth.make_pair(w, h, seed + k, noc)
        pairs.append((O.build_pyramid(p, ib), O.build_pyramid(p, ia)))
    return p, pairs


def _incoming(rng, w, h, scale=1.5):
    """test_stereo_varref_levels' incoming displacement: admissible (<= 0) values, a lattice of positive ones (clamped by the
    update) and one far outside the image (mask 0, clamped taps)."""
    flow = -np.abs(rand_planes(rng, h, w, 1, scale=scale))
    flow[::7, ::5] = 0.3
    flow[rng.integers(0, h), rng.integers(0, w)] = -3.0 * w
    return flow


def _varref_frames_vs_reference(gpu, p, pairs, nframes, rng, what, scale=1.5):
    """Frame k: pair k % 3 and an incoming displacement of its own, all frames in ONE device call; the reference frame by
    frame.  A frame that reads a neighbour's rows, system or displacement in a packed wavefront changes bits."""
    R = _ref(p.noc)
    flows = [_incoming(rng, p.width, p.height, scale) for _ in range(nframes)]
    im_a = np.stack([pairs[k % 3][0][0][0] for k in range(nframes)])
    im_b = np.stack([pairs[k % 3][1][0][0] for k in range(nframes)])
    got = gpu.varref_level(p, 0, im_a, im_b, np.stack(flows))
    for k in range(nframes):
        ref = R.varref_level(p, 0, im_a[k], im_b[k], flows[k])
        assert (ref <= 0).all()
        assert_bits_equal(got[k], ref, f"{what}: frame {k} of {nframes}")


# (w, h, channels, tv_innerit, tv_solverit, frames).  Rows: 4 (the fused kernel's least), 16 | 17 and 32 | 33 (16, 32 or 64
# lanes per frame: 4, 2 or 1 frames per wavefront), 64 | 65 (packed wavefronts | one workgroup per frame, the fused kernel's
# most), 128 | 129 (two | three wavefronts per workgroup); columns from 16 (the fused kernel's least); tv_solverit on both
# sides of 3 (the fused kernel's most) and of the sweeps one de_sor pass pipelines (4, or 3 above 64 rows); frame counts that
# leave the last wavefront and the last workgroup ragged.  The last one: more than 1024 rows, de_sor_serial_kernel.
# Every geometry went through the reference on a CPU first; it does not survive levels below 4 rows or 16 columns at this
# padding (15x3 segfaults inside the reference), so none is here.
BOUNDARY_LEVELS = [
    (16, 4, 1, 1, 1, 1), (17, 5, 1, 2, 3, 5), (31, 16, 1, 3, 4, 17), (33, 17, 1, 4, 5, 33), (64, 32, 1, 1, 9, 5),
    (65, 33, 1, 2, 1, 17), (100, 63, 1, 3, 3, 33), (16, 64, 1, 3, 4, 5), (17, 65, 1, 1, 3, 5), (31, 66, 1, 2, 4, 17),
    (33, 128, 1, 1, 5, 5), (64, 129, 1, 2, 9, 1), (65, 4, 1, 3, 3, 33), (100, 16, 1, 2, 2, 17), (64, 64, 1, 3, 3, 17),
    (65, 64, 3, 2, 3, 5), (100, 65, 1, 1, 4, 5), (33, 5, 3, 3, 2, 17), (17, 33, 3, 1, 5, 5), (31, 63, 1, 4, 9, 5),
    (16, 17, 1, 2, 1, 33), (100, 129, 3, 1, 3, 1), (64, 16, 1, 1, 4, 33), (17, 32, 1, 3, 1, 33), (33, 64, 1, 2, 5, 17),
    (65, 65, 1, 1, 9, 5), (16, 1030, 1, 1, 1, 1),
]


@pytest.mark.parametrize("w,h,noc,innerit,solverit,nframes", BOUNDARY_LEVELS,
                         ids=[f"{c[0]}x{c[1]}-noc{c[2]}-in{c[3]}-sor{c[4]}-f{c[5]}" for c in BOUNDARY_LEVELS])
def test_stereo_varref_boundary_levels(gpu, w, h, noc, innerit, solverit, nframes):
    """Stereo refinement levels on both sides of every size and sweep count the launchers switch on, distinct frames packed
    into wavefronts, bit for bit against the reference."""
    p, pairs = _free_level(w, h, noc, 15000 + 10 * w + h, tv_innerit=innerit, tv_solverit=solverit)
    rng = np.random.default_rng(15000 + 1000 * w + h)
    _varref_frames_vs_reference(gpu, p, pairs, nframes, rng, f"stereo level {w}x{h} noc={noc} innerit={innerit} solverit={solverit}")


@pytest.mark.parametrize("seed", range(24))
def test_random_stereo_varref_levels(gpu, seed):
    """test_gpu_kernels.py::test_random_varref_levels in stereo mode: random level geometry (from 16 columns and 4 rows, the
    reference's domain here), random TV parameters (tv_delta = 0: the instantiations without the brightness term), 1..9
    distinct frames."""
    rng = np.random.default_rng(16000 + seed + _SEED_OFFSET)
    noc = 3 if seed % 6 == 5 else 1
    w = int(rng.integers(16, 140))
    h = int(rng.integers(4, 65)) if seed % 7 else int(rng.integers(65, 150))
    if seed % 9 == 0:
        h = w = int(rng.integers(16, 65))
    over = dict(tv_innerit=int(rng.integers(1, 4)), tv_solverit=int(rng.integers(1, 5)),
                tv_sor=float(rng.choice([1.0, 1.6, 1.95])), tv_alpha=float(rng.choice([1.0, 10.0, 40.0])),
                tv_gamma=float(rng.choice([0.0, 10.0, 20.0])), tv_delta=float(rng.choice([0.0, 5.0, 15.0])))
    nframes = int(rng.integers(1, 10))
    p, pairs = _free_level(w, h, noc, 16100 + 3 * seed, **over)
    _varref_frames_vs_reference(gpu, p, pairs, nframes, rng, f"seed {seed}: {w}x{h} noc={noc} {over}",
                                scale=float(rng.choice([0.2, 1.5, 6.0])))


@pytest.mark.parametrize("seed", range(16))
def test_random_stereo_patchgrid_levels(gpu, seed):
    """test_gpu_kernels.py::test_random_patchgrid_levels in stereo mode: random patch size / overlap / iteration limits / cost
    function at one level, several distinct frames, with (odd seeds) and without a previous level's displacement -- which
    holds positive values, inadmissible for the left camera, and values that start patches outside the image."""
    rng = np.random.default_rng(17000 + seed + _SEED_OFFSET)
    noc = 3 if seed % 4 == 3 else 1
    P = int(rng.choice([4, 8, 8, 8, 12, 6]))
    w, h = int(rng.integers(max(3 * P, 16), 120)), int(rng.integers(3 * P, 90))
    w, h = w - w % 2, h - h % 2                                              # a coarser level of half the size exists
    over = dict(p_samp_s=P, patove=float(rng.choice([0.0, 0.4, 0.75])), max_iter=int(rng.integers(1, 14)),
                costfct=int(rng.integers(0, 3)), patnorm=int(rng.integers(0, 2)), res_thresh=float(rng.choice([0.0, 2.0])),
                dp_thresh=float(rng.choice([0.05, 0.3])), dr_thresh=float(rng.choice([0.95, 0.6])))
    over["min_iter"] = int(rng.integers(0, over["max_iter"] + 1))
    nframes = int(rng.integers(2, 6))
    p, pairs = _free_level(w, h, noc, 17100 + 3 * seed, **over)
    R = _ref(noc)
    prevs = None
    if seed % 2:
        prevs = []
        for _ in range(nframes):
            prev = -np.abs(rand_planes(rng, h // 2, w // 2, 1, scale=float(rng.choice([0.3, 2.0, 8.0]))))
            prev[::3, ::4] = 0.7                                             # positive: inadmissible for the left camera
            prev[0, 0] = -2.0 * w
            prev[-1, -1] = w
            prevs.append(prev)
    planes = [np.stack([pairs[k % 3][0][q][0] for k in range(nframes)]) for q in range(3)]
    im_b = np.stack([pairs[k % 3][1][0][0] for k in range(nframes)])
    gp, gflow = gpu.patchgrid_level(p, 0, planes[0], planes[1], planes[2], im_b, np.stack(prevs) if prevs else None)
    what = f"seed {seed}: {w}x{h} P={P} noc={noc} frames={nframes} prev={'yes' if prevs else 'no'} {over}"
    for k in range(nframes):
        rp, rflow = R.patchgrid_level(p, 0, planes[0][k], planes[1][k], planes[2][k], im_b[k], prevs[k] if prevs else None)
        assert rflow.shape[-1] == 1
        # left camera: disparity <= 0 (patch.cpp:190) -- imposed on every UPDATE: a patch that starts outside the image (:135) or
        # is reset to its start as an outlier (:199-207) keeps an inadmissible start value in the reference itself, so the
        # constraint is asserted where every patch starts at 0; with a previous level the reference's bits decide
        assert (rp[:, 1] == 0).all() and (gp[k][:, 1] == 0).all(), what + f": frame {k}, vertical component"
        if not prevs:
            assert (rp[:, 0] <= 0).all() and (gp[k][:, 0] <= 0).all(), what + f": frame {k}, left camera's constraint"
        assert_bits_equal(gp[k], rp, what + f": patch displacements, frame {k}")
        assert_bits_equal(gflow[k], rflow, what + f": dense displacement, frame {k}")
