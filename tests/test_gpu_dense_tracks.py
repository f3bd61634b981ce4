"""-m gpu: dense trajectories (include/ofdis.h: ofdis_seed_texture, ofdis_dense_tracks on materialised flows,
ofdis_batch_dense_tracks straight from the level flows of a sequence context).

The texture test is compared byte for byte and the standalone call bit for bit -- tracks, start, len, info -- with
of_dis_amd/tracking.py (seed_texture_ref, dense_tracks_ref: the header's definition in numpy); the batch form bit for bit with
the standalone call applied to what ofdis_batch_upsample_bidir / ofdis_batch_upsample_frames write.  Conditions on the generated
inputs (tracks end in every way, seeds are dropped, enough tracks survive) are checked on the restatement or the standalone
result, never on the kernel under test."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gen_synth
from of_dis_amd import tracking
from seq_products import INVALID, assert_same_bits, flag_contexts, run_context, smooth_clip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f32 = np.float32
T_MAX = 2 ** 31 - 1


def assert_dense_equal(got, want, what):
    """(tracks, start, len, info) of two runs: info first (it says how many slots there are), then every slot bit for bit"""
    (gt, gs, gl, gi), (wt, ws, wl, wi) = got, want
    assert np.array_equal(gi, wi), (what, "info", gi, wi)
    assert gt.shape == wt.shape and gs.shape == ws.shape and gl.shape == wl.shape, (what, gt.shape, wt.shape)
    for name, g, w in (("start", gs, ws), ("len", gl, wl)):
        if not np.array_equal(g, w):
            i = int(np.flatnonzero(g != w)[0])
            raise AssertionError(f"{what}: {(g != w).sum()} of {g.size} {name} values differ; first at slot {i}: {g[i]} vs {w[i]}")
    assert_same_bits(gt, wt, what + ", tracks [step][slot][component]")


def _threshold(frame0, stride, window, share):
    """the largest T for which at least `share` of frame 0's cells are textured (bisection on the restatement)"""
    textured = lambda T: tracking.seed_texture_ref(frame0[None], stride, window, T).mean() >= share
    assert textured(0)
    lo, hi = 0, T_MAX
    if textured(hi):
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if textured(mid) else (lo, mid)
    return lo


# ------------------------------------------------------------------ 1. the texture test against the restatement
TEXTURE_SIZES = [(64, 48), (37, 11), (67, 45), (9, 7), (5, 2)]


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", TEXTURE_SIZES, ids=[f"{w}x{h}" for w, h in TEXTURE_SIZES])
def test_seed_texture_matches_the_definition(gpu, w, h, noc):
    """frames: gen_synth's texture (both images of a pair), uniform random bytes (the largest sums), a constant frame"""
    rng = np.random.default_rng(100 * w + h + noc)
    a, b, _ = gen_synth.make_pair(w, h, 6200, noc)
    shape = a.shape
    frames = np.stack([a, b, rng.integers(0, 256, shape).astype(np.uint8), np.full(shape, 77, np.uint8)])
    mixed = 0
    for stride in (2, 3, 5, 4):
        if stride > min(w, h):
            continue
        for window in (0, 1, 2, 7):
            ta, tb, tc = tracking.structure_tensor(frames[:1], stride, window)
            lam = ((ta + tc) - np.sqrt((ta - tc).astype(np.float64) ** 2 + 4.0 * tb.astype(np.float64) ** 2)) / 2
            for T in (0, max(1, int(np.median(lam))), T_MAX):
                want = tracking.seed_texture_ref(frames, stride, window, T)
                got = gpu.seed_texture(frames, stride, window, T)
                assert got.dtype == np.uint8 and got.shape == want.shape
                assert np.array_equal(got, want), (stride, window, T, int((got != want).sum()), want.size)
                # conditions on the inputs, from the restatement
                assert want[:3].all() if T == 0 else not want[3].any(), (stride, window, T)
                if T == 0:
                    assert want.all()
                elif T < T_MAX:
                    mixed += 0 < want[:3].sum() < want[:3].size
    assert mixed or w * h < 100, "the mid threshold never separated the cells"


# ------------------------------------------------------------------ 2. the standalone call against the restatement
@functools.lru_cache(maxsize=None)
def _recipe(w, h, noc, stride, window, npairs):
    """frames of one texture rolled by a pixel per frame with a flat patch in a corner; a flow of about (1.25, -0.5) with a NaN;
    a reverse flow that contradicts it in the lower right quadrant.  T: the largest value that leaves 60 % of frame 0's cells
    textured."""
    base = gen_synth.make_pair(w, h, 6200, noc)[0]
    frames = np.stack([np.roll(base, k, axis=1) for k in range(npairs + 1)])
    frames[:, :h // 3, :w // 3] = 128
    T = _threshold(frames[0], stride, window, 0.6)
    ys, xs = np.mgrid[0:h, 0:w]
    fw = np.empty((npairs, h, w, 2), _f32)
    fw[..., 0] = (1.25 + 0.05 * np.sin(xs / 7)).astype(_f32)
    fw[..., 1] = -0.5
    rev = -fw
    rev[:, h // 2:, w // 2:] += 1.5
    fw[1, 3, 5] = np.nan
    return np.ascontiguousarray(frames), fw, rev, T


# (w, h, stride, window, npairs, max_len)
DENSE_CASES = [(64, 48, 2, 1, 6, 0), (64, 48, 2, 1, 6, 2), (37, 11, 3, 2, 5, 3), (67, 45, 5, 2, 6, 4), (9, 7, 4, 0, 3, 1)]
DENSE_IDS = [f"{c[0]}x{c[1]}-s{c[2]}-w{c[3]}-n{c[4]}-L{c[5]}" for c in DENSE_CASES]
# what the numpy model gave for the 64x48 gray cases when the recipe was written: (ntracks, reseeds, outside, inconsistent,
# complete, dropped at half capacity)
MODEL_64x48 = {0: (1333, 868, 72, 741, 283, 801), 2: (1929, 1464, 45, 737, 1013, 1321)}


@pytest.mark.parametrize("with_rev", [True, False], ids=["rev", "fw-only"])
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h,stride,window,npairs,max_len", DENSE_CASES, ids=DENSE_IDS)
def test_dense_tracks_match_the_definition(gpu, w, h, stride, window, npairs, max_len, noc, with_rev):
    frames, fw, rev, T = _recipe(w, h, noc, stride, window, npairs)
    r = rev if with_rev else None
    why = {}
    want = tracking.dense_tracks_ref(frames, fw, r, stride, window, T, max_len, reasons=why)
    n = int(want[3][0])
    # conditions on the inputs, from the restatement
    assert why["dropped"] == 0 and n > 0
    if with_rev:
        # (9x7 with max_len 1: every track is one step of about (1.25, -0.5) from a centre at least 2 px inside, none can leave)
        ways = ("inconsistent", "reseeds", "complete") + (("outside",) if (w, h) != (9, 7) else ())
        assert all(why[k] > 0 for k in ways), why
        if (w, h, noc) == (64, 48, 1):
            assert (n, why["reseeds"], why["outside"], why["inconsistent"], why["complete"]) == MODEL_64x48[max_len][:5]
    assert_dense_equal(gpu.dense_tracks(frames, fw, r, stride, window, T, max_len), want, "ample")
    assert_dense_equal(gpu.dense_tracks(frames, fw, r, stride, window, T, max_len, max_tracks=n + 7), want, "seven spare slots")
    why = {}
    want = tracking.dense_tracks_ref(frames, fw, r, stride, window, T, max_len, max_tracks=n // 2, reasons=why)
    assert why["dropped"] > 0 and want[3][0] == n // 2
    if with_rev and (w, h, noc) == (64, 48, 1):
        assert why["dropped"] == MODEL_64x48[max_len][5]
    assert_dense_equal(gpu.dense_tracks(frames, fw, r, stride, window, T, max_len, max_tracks=n // 2), want, "half capacity")


def _wild_flows(rng, w, h, npairs):
    """the "wild" recipe of tests/test_gpu_track.py: normal flows of 3 px with large, infinite, NaN and image-sized values
    mixed in"""
    F = [(rng.standard_normal((npairs, h, w, 2)) * 3).astype(_f32) for _ in range(2)]
    for f in F:
        pick = rng.random((npairs, h, w, 2))
        f[pick < 0.08] = (rng.standard_normal(int((pick < 0.08).sum())) * 1e4).astype(_f32)
        f[(pick >= 0.08) & (pick < 0.1)] = np.inf
        f[(pick >= 0.1) & (pick < 0.12)] = -np.inf
        f[(pick >= 0.12) & (pick < 0.14)] = np.nan
        sized = (pick >= 0.14) & (pick < 0.2)
        f[sized] = (rng.uniform(-2, 2, int(sized.sum())) * max(w, h)).astype(_f32)
    return F[0], F[1]


@pytest.mark.parametrize("max_len", [0, 2])
def test_dense_tracks_on_wild_flows(gpu, max_len):
    w, h, npairs = 37, 11, 5
    frames, _, _, T = _recipe(w, h, 1, 3, 2, npairs)
    fw, rev = _wild_flows(np.random.default_rng(3711), w, h, npairs)
    for r in (rev, None):
        for alpha, beta in ((tracking.FB_ALPHA, tracking.FB_BETA), (0.2, 3.0)):
            why = {}
            want = tracking.dense_tracks_ref(frames, fw, r, 3, 2, T, max_len, alpha=alpha, beta=beta, reasons=why)
            assert why["outside"] > 0 and why["reseeds"] > 0 and (r is None or why["inconsistent"] > 0), why
            assert_dense_equal(gpu.dense_tracks(frames, fw, r, 3, 2, T, max_len, alpha=alpha, beta=beta), want, f"wild {alpha} {beta}")


def test_known_count(gpu):
    """T = 0, zero flows: every cell seeds at frame 0 and again whenever its track is complete"""
    w, h, npairs, stride = 37, 11, 5, 3
    frames, fw, _, _ = _recipe(w, h, 1, stride, 2, npairs)
    ncx, ncy = tracking.dense_grid(w, h, stride)
    for max_len in (0, 1, 2, 5, 9):
        lmax = min(max_len, npairs) if max_len else npairs
        tracks, start, length, info = gpu.dense_tracks(frames, np.zeros_like(fw), np.zeros_like(fw), stride, 2, 0, max_len)
        assert info.tolist() == [ncx * ncy * -(-npairs // lmax), 0]
        assert (length[start + lmax <= npairs] == lmax + 1).all() and (length[start + lmax > npairs] == npairs - start[start + lmax > npairs] + 1).all()


# ------------------------------------------------------------------ 3. every entry written, nothing else written
@pytest.mark.parametrize("with_len", [True, False])
@pytest.mark.parametrize("capped", [False, True])
def test_every_entry_is_written_and_nothing_else(gpu, with_len, capped):
    w, h, stride, window, npairs, max_len, guard = 64, 48, 2, 1, 6, 2, 4096
    frames, fw, rev, T = _recipe(w, h, 1, stride, window, npairs)
    full = int(tracking.dense_tracks_ref(frames, fw, rev, stride, window, T, max_len)[3][0])
    max_tracks = full // 2 if capped else full + 100
    want = tracking.dense_tracks_ref(frames, fw, rev, stride, window, T, max_len, max_tracks=max_tracks)
    n, lmax = int(want[3][0]), max_len
    sizes = dict(tracks=(lmax + 1) * max_tracks * 8, start=max_tracks * 4, len=max_tracks * 4, info=16)
    dev = {k: gpu.Dev(np.full(v + guard, 0xAB, np.uint8)) for k, v in sizes.items()}
    dfr, dfw, drev = gpu.Dev(frames), gpu.Dev(fw), gpu.Dev(rev)
    wb = gpu.lib().ofdis_dense_tracks_work_bytes(npairs, w, h, stride)
    dwork = gpu.Dev(np.full(wb + guard, 0xAB, np.uint8))
    gpu.check(gpu.lib().ofdis_dense_tracks(dfr.ptr, dfw.ptr, drev.ptr, npairs, w, h, 1, stride, window, T, max_len, gpu.FB_ALPHA,
                                           gpu.FB_BETA, max_tracks, dev["tracks"].ptr, dev["start"].ptr,
                                           dev["len"].ptr if with_len else None, dev["info"].ptr, dwork.ptr, wb, None))
    gpu.check(gpu.lib().ofdis_sync(None))
    raw = {k: dev[k].get((v + guard,), np.uint8) for k, v in sizes.items()}
    for k, v in sizes.items():
        assert (raw[k][v:] == 0xAB).all(), f"guard behind {k}"
    assert (dwork.get((wb + guard,), np.uint8)[wb:] == 0xAB).all(), "guard behind work"
    info = raw["info"][:16].view(np.int64)
    assert np.array_equal(info, want[3])
    tracks = raw["tracks"][:sizes["tracks"]].view(np.uint32).reshape(lmax + 1, max_tracks, 2)
    start, length = raw["start"][:sizes["start"]].view(np.uint32), raw["len"][:sizes["len"]].view(np.uint32)
    assert (tracks[:, n:] == 0xABABABAB).all() and (start[n:] == 0xABABABAB).all() and (length[n:] == 0xABABABAB).all()
    assert not (tracks[:, :n] == 0xABABABAB).any() and not (start[:n] == 0xABABABAB).any()
    if with_len:
        assert not (length[:n] == 0xABABABAB).any()
        got = (tracks[:, :n].view(_f32), start[:n].view(np.int32), length[:n].view(np.int32), info)
        assert_dense_equal(got, want, "guarded")
    else:
        assert (length == 0xABABABAB).all()
        assert_same_bits(tracks[:, :n].view(_f32), want[0], "len = NULL, tracks")
        assert np.array_equal(start[:n].view(np.int32), want[1])


# ------------------------------------------------------------------ 4. replay through ofdis_track_points
@pytest.mark.parametrize("with_rev", [True, False], ids=["rev", "fw-only"])
def test_every_slot_replays_through_track_points(gpu, with_rev):
    w, h, stride, window, npairs, max_len = 67, 45, 5, 2, 6, 4
    frames, fw, rev, T = _recipe(w, h, 1, stride, window, npairs)
    r = rev if with_rev else None
    tracks, start, length, info = gpu.dense_tracks(frames, fw, r, stride, window, T, max_len)
    n = int(info[0])
    assert n > 0 and (start > 0).any()
    replay, counts = gpu.track_points(fw, r, tracks[0], start, max_steps=max_len)
    assert np.array_equal(counts, length)
    assert_same_bits(replay, tracking.to_frame_major(tracks, start, length, npairs), "replay")


# ------------------------------------------------------------------ 5. the batch form against the standalone call
def _clip_threshold(frames, stride, window):
    """a T that 50 - 90 % of frame 0's cells pass (checked on the restatement)"""
    T = _threshold(frames[0], stride, window, 0.7)
    share = tracking.seed_texture_ref(frames[:1], stride, window, T).mean()
    assert 0.5 <= share <= 0.9, share
    return T


# (noc, w, h, n pairs, contract, pipeline): the contexts of tests/test_gpu_track.py
FUSED_CASES = [
    pytest.param(1, 256, 112, 3, 0, 1, id="gray-256x112-n3-exact"),
    pytest.param(1, 256, 112, 5, 1, 1, id="gray-256x112-n5-fused"),
    pytest.param(1, 250, 107, 5, 0, 1, id="gray-250x107-n5-exact"),
    pytest.param(1, 250, 107, 3, 1, 1, id="gray-250x107-n3-fused"),
    pytest.param(3, 256, 112, 3, 0, 1, id="rgb-256x112-n3-exact"),
    pytest.param(1, 256, 112, 5, 0, 2, id="gray-256x112-n5-exact-pipelined"),
]
STRIDE, WINDOW = 5, 2


@pytest.mark.parametrize("noc,w,h,n,contract,pipeline", FUSED_CASES)
def test_batch_form_matches_standalone_on_the_materialised_flows(gpu, noc, w, h, n, contract, pipeline):
    """max_len 0 and 2, with the consistency test (against upsample_bidir's two flows) and without it, the full range and the
    sub-range (1, n - 1)"""
    frames = smooth_clip(w, h, noc, n + 1)
    T = _clip_threshold(frames, STRIDE, WINDOW)
    b, (d,) = run_context(gpu, frames, "seq_rev", contract=contract, pipeline=pipeline)
    try:
        before = b.device_bytes()
        fused = {(first, count, fb, ml): b.dense_tracks(d.ptr, w, h, STRIDE, WINDOW, T, ml, fb_check=fb, first=first, count=count)
                 for first, count in ((0, n), (1, n - 1)) for fb in (True, False) for ml in (0, 2)}
        assert b.device_bytes() > before  # the work buffer belongs to the context
        fw, rev, _, _ = b.upsample_bidir(w, h, outputs=(True, True, False, False))
    finally:
        b.close()
    for (first, count, fb, ml), got in fused.items():
        sl = slice(first, first + count)
        want = gpu.dense_tracks(frames[first:first + count + 1], fw[sl], rev[sl] if fb else None, STRIDE, WINDOW, T, ml)
        assert_dense_equal(got, want, f"pairs [{first}, {first + count}), fb_check {fb}, max_len {ml}")
    # the clip is gentle enough for the comparison to cover whole tracks (condition on the standalone result)
    _, start, length, _ = gpu.dense_tracks(frames, fw, rev, STRIDE, WINDOW, T, 0)
    first_generation = start == 0
    assert first_generation.any() and 2 * (length[first_generation] == n + 1).sum() >= first_generation.sum()


@pytest.mark.parametrize("contract", [0, 1], ids=["exact", "fused"])
def test_batch_form_without_the_test_on_a_forward_only_sequence(gpu, contract):
    w, h, n = 250, 107, 3
    frames = smooth_clip(w, h, 1, n + 1)
    T = _clip_threshold(frames, STRIDE, WINDOW)
    b, (d,) = run_context(gpu, frames, "seq", contract=contract)
    try:
        got = b.dense_tracks(d.ptr, w, h, STRIDE, WINDOW, T, 2, fb_check=False)
        fw = b.upsample_frames(0, n, w, h)
    finally:
        b.close()
    assert_dense_equal(got, gpu.dense_tracks(frames, fw, None, STRIDE, WINDOW, T, 2), "forward-only sequence context")


def test_batch_form_grows_its_work_buffer(gpu):
    """one pair first, then all n: the second call needs more than the first left, allocates again and gives what a context
    that never held the smaller buffer gives; a call that needs no more allocates nothing"""
    w, h, n = 250, 107, 3
    frames = smooth_clip(w, h, 1, n + 1)
    T = _clip_threshold(frames, STRIDE, WINDOW)
    b, (d,) = run_context(gpu, frames)
    try:
        sizes = [b.device_bytes()]
        b.dense_tracks(d.ptr, w, h, STRIDE, WINDOW, T, first=0, count=1)
        sizes.append(b.device_bytes())
        grown = b.dense_tracks(d.ptr, w, h, STRIDE, WINDOW, T, first=0, count=n)
        sizes.append(b.device_bytes())
        b.dense_tracks(d.ptr, w, h, STRIDE, WINDOW, T, first=0, count=n)
        sizes.append(b.device_bytes())
    finally:
        b.close()
    assert sizes[0] < sizes[1] < sizes[2] == sizes[3], sizes
    fresh, (d,) = run_context(gpu, frames)
    try:
        want = fresh.dense_tracks(d.ptr, w, h, STRIDE, WINDOW, T, first=0, count=n)
    finally:
        fresh.close()
    assert_dense_equal(grown, want, "after the work buffer grew")


# ------------------------------------------------------------------ 6. checks that need a context
@pytest.fixture(scope="module")
def contexts(gpu):
    yield from flag_contexts(gpu)


def _batch_call(gpu, b, frames=True, first=0, count=3, stride=5, window=2, min_eig=10, max_len=2, fb_check=1, alpha=0.01,
                beta=0.5, max_tracks=64, tracks=True, start=True, info=True, wo=256, ho=112):
    """host buffers stand in for the device arrays: every call returns before it would launch"""
    fr, t, s, i = np.zeros(16, np.uint8), np.zeros((4, 64, 2), _f32), np.zeros(64, np.int32), np.zeros(2, np.int64)
    p = lambda a, on: a.ctypes.data if on else None
    return gpu.lib().ofdis_batch_dense_tracks(b.h, p(fr, frames), first, count, stride, window, min_eig, max_len, fb_check, alpha,
                                              beta, max_tracks, p(t, tracks), p(s, start), None, p(i, info), wo, ho, None)


@pytest.mark.parametrize("which", ["plain", "reverse"])
def test_batch_dense_tracks_needs_a_sequence_context(gpu, contexts, which):
    assert _batch_call(gpu, contexts[which]) == INVALID
    assert "SEQUENCE" in gpu.lib().ofdis_last_error().decode()


def test_batch_dense_tracks_with_the_test_needs_a_reverse_context(gpu, contexts):
    assert _batch_call(gpu, contexts["seq"], fb_check=1) == INVALID
    assert "REVERSE" in gpu.lib().ofdis_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(first=-1), None), (dict(count=0), None), (dict(first=1, count=3), None), (dict(first=3, count=1), None),
    (dict(count=4), None), (dict(wo=0), None), (dict(ho=0), None), (dict(wo=257), None), (dict(ho=113), None),
    (dict(fb_check=2), "fb_check"), (dict(fb_check=-1), "fb_check"), (dict(frames=False), "frames"), (dict(tracks=False), "tracks"),
    (dict(start=False), "start"), (dict(info=False), "info"), (dict(stride=1), "stride"), (dict(stride=65), "stride"),
    (dict(stride=64, wo=63), "stride"), (dict(stride=64, ho=63), "stride"), (dict(window=-1), "window"),
    (dict(window=8), "window"), (dict(min_eig=-1), "min_eig"), (dict(max_len=-1), "max_len"), (dict(max_tracks=0), "max_tracks"),
    (dict(max_tracks=(1 << 24) + 1), "max_tracks"), (dict(alpha=-0.01), "alpha"), (dict(beta=float("nan")), "alpha"),
], ids=lambda v: ",".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else "")
def test_batch_dense_tracks_rejects(gpu, contexts, kw, word):
    assert _batch_call(gpu, contexts["seq_rev"], **kw) == INVALID
    msg = gpu.lib().ofdis_last_error().decode()
    assert msg and (word is None or word in msg), msg


# ------------------------------------------------------------------ 7. the command-line tool
def test_flow_images_dense_tracks(gpu, tmp_path):
    """tools/flow_images.py --sequence --reverse --dense-tracks 5:2:T:3: <stem>_dtracks.npy, _dstart.npy and _dlen.npy hold
    what the standalone call makes of the .flo / .rev.flo files the same run writes; without --sequence it is refused"""
    from PIL import Image
    w, h, n = 250, 107, 3
    frames = smooth_clip(w, h, 1, n + 1)
    T = _clip_threshold(frames, STRIDE, WINDOW)
    paths = []
    for k, f in enumerate(frames):
        paths.append(str(tmp_path / f"f{k}.png"))
        Image.fromarray(f).save(paths[-1])
    tool, stem = os.path.join(ROOT, "tools", "flow_images.py"), str(tmp_path / "clip")
    run = lambda args: subprocess.run([sys.executable, tool] + args, capture_output=True, text=True, timeout=300)
    res = run(["--sequence", "--reverse", "--dense-tracks", f"5:2:{T}:3"] + paths + [stem])
    assert res.returncode == 0, (res.stdout, res.stderr)
    read_flo = lambda path: np.fromfile(path, _f32, offset=12).reshape(h, w, 2)
    fw = np.stack([read_flo(f"{stem}_{k:03d}.flo") for k in range(n)])
    rev = np.stack([read_flo(f"{stem}_{k:03d}.rev.flo") for k in range(n)])
    tracks, start, length = (np.load(stem + f"_{name}.npy") for name in ("dtracks", "dstart", "dlen"))
    assert tracks.dtype == _f32 and start.dtype == np.int32 and length.dtype == np.int32
    want = gpu.dense_tracks(frames, fw, rev, 5, 2, T, 3)
    assert_dense_equal((tracks, start, length, want[3]), want, "the tool's files")
    res = run(["--reverse", "--dense-tracks", "5"] + paths[:2] + [stem + ".flo"])
    assert res.returncode != 0 and "--sequence" in (res.stderr + res.stdout)
