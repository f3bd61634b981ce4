"""What the GPU tests of the sequence products (tests/test_gpu_interp.py, _track, _dense_tracks, _tfilter, _trajfilter, _gmotion,
_stabilize) and of the contexts under them (_bidir, _stereo_lr, _seq) share: the clip, a context built over it and run, the
bit-pattern comparison, the unfilled contexts of the rejection tests with the cases every product rejects alike, and the
level-flow helpers.  A new product's test starts here; what names one product's outputs or one C signature stays in its file."""
import functools
import math

import numpy as np

import gen_synth
from common import assert_bits_equal
from of_dis_amd.params import oppoint, padded_size

INVALID = -1
FLT_MIN = float(np.finfo(np.float32).tiny)


# ------------------------------------------------------------------ the clip
CLIP_STEP = 0.15  # of gen_synth's flow (up to 12 px) per frame: at most 1.8 px per pair, 9 px over five pairs


@functools.lru_cache(maxsize=None)
def smooth_clip(w, h, noc, nframes, seed=6200, step=CLIP_STEP, walk=None):
    """nframes frames [nframes][h][w] (+ [3]) uint8 of one scene in smooth motion: gen_synth's texture displaced by walk[k] * step
    of its flow in frame k; walk = None: 0, 1, 2, ...  Cached and shared between the files, so read-only."""
    walk = range(nframes) if walk is None else walk[:nframes]
    assert len(walk) == nframes and walk[0] == 0
    frames = [gen_synth.make_pair(w, h, seed, noc)[0]]
    frames += [gen_synth.make_pair(w, h, seed, noc, flow_scale=step * k)[1] for k in walk[1:]]
    out = np.ascontiguousarray(np.stack(frames))
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------ a context over a clip, built and run
def run_context(gpu, clip, kind="seq_rev", opp=2, contract=0, pipeline=1):
    """a context over the pairs of the clip [n + 1][h][w] (+ [3]), built and run.  kind: "plain" and "reverse" hold every pair's
    two frames (A = clip[:-1], B = clip[1:]), "seq" and "seq_rev" are SEQUENCE contexts (the latter | REVERSE) over the clip
    itself.  Returns (context, the device arrays it reads: [A, B] or [clip])."""
    n, h, w = clip.shape[0] - 1, clip.shape[1], clip.shape[2]
    noc = 1 if clip.ndim == 3 else 3
    sequence, reverse = {"plain": (False, False), "reverse": (False, True), "seq": (True, False), "seq_rev": (True, True)}[kind]
    p = oppoint(opp, w, h, noc=noc, verbosity=0)
    p.width, p.height = padded_size(w, h, p.sc_f)
    devs = [gpu.Dev(clip)] if sequence else [gpu.Dev(clip[:-1]), gpu.Dev(clip[1:])]
    old = gpu.set_tuning(contract=contract)
    try:
        b = gpu.Batch(p, n, sequence=sequence, reverse=reverse)
        if pipeline > 1:
            b.set_pipeline(pipeline)
        if sequence:
            b.build_pyramids_u8_seq(devs[0].ptr, w, h)
        else:
            b.build_pyramids_u8(devs[0].ptr, devs[1].ptr, w, h)
        b.run()
    finally:
        gpu.restore_tuning(old)
    return b, devs


# ------------------------------------------------------------------ the comparison
def assert_same_bits(got, want, what):
    """arrays of one shape and one dtype compared as raw bit patterns: -0 is not +0, a NaN equals only its own payload
    (common.assert_bits_equal compares float32 by value)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bits = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    g, w = np.ascontiguousarray(got).view(bits), np.ascontiguousarray(want).view(bits)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ; first at {i}: {got[i]!r} ({g[i]:#x}) vs "
                             f"{want[i]!r} ({w[i]:#x})")


# ------------------------------------------------------------------ the checks that need a context and nothing in it
def flag_contexts(gpu, stereo=False):
    """yields {name: an unfilled context of 3 pairs at oppoint(2, 256, 112)}, one per combination of creation flags ("plain",
    "reverse", "seq", "seq_rev"; stereo: "stereo" and "stereo_lr" as well), and closes them: the body of a module's fixture"""
    p = oppoint(2, 256, 112)
    made = dict(plain=gpu.Batch(p, 3), reverse=gpu.Batch(p, 3, reverse=True), seq=gpu.Batch(p, 3, sequence=True),
                seq_rev=gpu.Batch(p, 3, sequence=True, reverse=True))
    if stereo:
        made.update(stereo=gpu.Batch(p.copy(selectmode=2), 3), stereo_lr=gpu.Batch(p.copy(selectmode=2), 3, stereo_lr=True))
    yield made
    for b in made.values():
        b.close()


# keyword arguments of a file's _batch_call on such a context (3 pairs, padded to 256 x 112) that every product must reject
RANGE_REJECTS = [dict(first=-1), dict(count=0), dict(count=-1), dict(first=1, count=3), dict(first=3, count=1), dict(count=4)]
SIZE_REJECTS = [dict(wo=0), dict(ho=0), dict(wo=257), dict(ho=113)]
FB_REJECTS = [dict(alpha=-0.01), dict(beta=-0.5), dict(alpha=math.nan), dict(beta=math.inf)]


# ------------------------------------------------------------------ level flows
def fill_u8(gpu, b, ia, ib, w, h):
    da, db = gpu.Dev(ia), gpu.Dev(ib)
    b.build_pyramids_u8(da.ptr, db.ptr, w, h)
    gpu.check(gpu.lib().ofdis_sync(None))
    da.free()
    db.free()


def levels(b, p, which="forward"):
    """{level: its flow}; which: "forward", "reverse" (REVERSE contexts) or "mirror" (STEREO_LR contexts)"""
    read = {"forward": b.level_flow, "reverse": b.level_flow_reverse, "mirror": b.level_flow_mirror}[which]
    return {l: read(l) for l in range(p.sc_l, p.sc_f + 1)}


def check_levels(got, want, what):
    for l in want:
        assert_bits_equal(got[l], want[l], f"{what}, level {l}")
