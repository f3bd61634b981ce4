"""-m gpu: video sequence contexts (ofdis_batch_create_ex with OFDIS_BATCH_SEQUENCE): n + 1 frames give n pairs, every
frame's planes are built and held once, B's planes are A's one frame further on.

The numerical path is the plain context's, so every comparison is bit for bit against a context that does not share
anything: a plain (or OFDIS_BATCH_REVERSE) context fed img_a = frames[:-1], img_b = frames[1:]."""
import functools

import numpy as np
import pytest

import gen_synth
import oracle
from common import assert_bits_equal
from of_dis_amd.params import oppoint, padded_size
from seq_products import check_levels, fill_u8, levels

pytestmark = pytest.mark.gpu
_f32 = np.float32


# ------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=8)
def _base_frames(w, h, noc, seed=5100):
    """Four frames of one scene in motion: the texture of `seed` displaced by 0, 1/2, 1 and 3/2 of the synthetic flow."""
    out = [gen_synth.make_pair(w, h, seed, noc)[0]]
    out += [gen_synth.make_pair(w, h, seed, noc, flow_scale=0.5 * k)[1] for k in (1, 2, 3)]
    return tuple(out)


def _frames(w, h, noc, count):
    """count frames [count][h][w]([3]) uint8; longer clips play the four frames forth and back (no pair is (X, X))"""
    base = _base_frames(w, h, noc)
    walk = [0, 1, 2, 3, 2, 1]
    return np.ascontiguousarray(np.stack([base[walk[k % 6]] for k in range(count)]))


def _params(opp, w, h, noc=1, tv=1, fb=0):
    p = oppoint(opp, w, h, noc=noc, usetvref=tv).copy(usefbcon=fb)
    p.width, p.height = padded_size(w, h, p.sc_f)
    return p


def _sync(gpu):
    gpu.check(gpu.lib().ofdis_sync(None))


def _fill_pairs(gpu, b, frames, w, h):
    """a plain / reverse context from the same clip, the parent's way: every interior frame twice"""
    fill_u8(gpu, b, frames[:-1], frames[1:], w, h)


def _fill_seq(gpu, b, frames, w, h):
    d = gpu.Dev(frames)
    b.build_pyramids_u8_seq(d.ptr, w, h)
    _sync(gpu)
    d.free()


def _host_pyramids(p, frames):
    O = oracle.c_oracle()
    return [O.build_pyramid(p, f) for f in frames]


def _planes(gpu, b, p, kind, nframes):
    """input planes of `kind`, `nframes` frames from the pointer ofdis_batch_input returns, per level"""
    out = {}
    for l in range(p.sc_l, p.sc_f + 1):
        ptr = b.input_ptr(l, kind)
        assert ptr, (l, kind)
        a = np.empty((nframes, b.input_elems(l)), _f32)
        gpu.check(gpu.lib().ofdis_memcpy_d2h(a.ctypes.data, ptr, a.nbytes))
        out[l] = a
    return out


# ------------------------------------------------------------------ 1. every level, both directions
# (noc, op, usefbcon, tv, n pairs, fill, width, height)
SEQ_CASES = [
    pytest.param(1, 2, 0, 1, 3, "u8", 256, 112, id="gray-op2-tv-n3-u8"),
    pytest.param(1, 2, 0, 0, 1, "u8", 256, 112, id="gray-op2-notv-n1-u8"),
    pytest.param(1, 2, 1, 1, 3, "u8", 256, 112, id="gray-op2-fb-n3-u8"),
    pytest.param(3, 2, 0, 1, 3, "u8", 256, 112, id="rgb-op2-tv-n3-u8"),
    pytest.param(1, 3, 0, 1, 1, "host", 320, 240, id="gray-op3-n1-host"),
    # more pairs than the small-batch mappings of the fused TV kernel take: the strip mapping sees B pointers that are A's
    # shifted by one frame
    pytest.param(1, 2, 0, 1, 800, "u8", 256, 112, id="gray-op2-tv-n800-u8-strips"),
]


@pytest.mark.parametrize("contract", [0, 1], ids=["exact", "fused"])
@pytest.mark.parametrize("noc,opp,fb,tv,n,fill,w,h", SEQ_CASES)
def test_sequence_equals_pairwise_contexts(gpu, contract, noc, opp, fb, tv, n, fill, w, h):
    """Every level of the forward flow (a forward-only and a reverse sequence context) and of the reverse flow of pair k ==
    what an OFDIS_BATCH_REVERSE context computes for (frame k, frame k + 1)."""
    p = _params(opp, w, h, noc, tv, fb)
    frames = _frames(w, h, noc, n + 1)
    old = gpu.set_tuning(contract=contract)
    try:
        ref = gpu.Batch(p, n, reverse=True)
        sr = gpu.Batch(p, n, sequence=True, reverse=True)
        sf = gpu.Batch(p, n, sequence=True)
        if fill == "u8":
            _fill_pairs(gpu, ref, frames, w, h)
            _fill_seq(gpu, sr, frames, w, h)
            _fill_seq(gpu, sf, frames, w, h)
        else:
            pyr = _host_pyramids(p, frames)
            for k in range(n):
                ref.upload(k, pyr[k][0], pyr[k][1], pyr[k][2], pyr[k + 1][0])
                ref.upload_b_gradients(k, pyr[k + 1][1], pyr[k + 1][2])
            for b in (sr, sf):
                for k in range(n + 1):
                    b.upload_frame(k, pyr[k][0], pyr[k][1], pyr[k][2])
        for b in (ref, sr, sf):
            b.run()
        want_fw, want_rev = levels(ref, p), levels(ref, p, "reverse")
        check_levels(levels(sr, p), want_fw, "forward flow, sequence + reverse context")
        check_levels(levels(sr, p, "reverse"), want_rev, "reverse flow, sequence + reverse context")
        check_levels(levels(sf, p), want_fw, "forward flow, forward-only sequence context")
        assert sr.status() == 0 and sf.status() == 0
        assert not np.array_equal(want_fw[p.sc_l], want_rev[p.sc_l])
        if n > 1:
            assert not np.array_equal(want_fw[p.sc_l][0], want_fw[p.sc_l][1])
        for b in (ref, sr, sf):
            b.close()
    finally:
        gpu.restore_tuning(old)


# ------------------------------------------------------------------ 2. frame views of aliased planes, graph replay, warm start
@pytest.fixture(scope="module")
def gray_ref(gpu):
    """{n: (params, frames, forward levels, reverse levels)} of the gray op-2 clip on a reverse context, computed once"""
    w, h = 256, 112
    p = _params(2, w, h)
    out = {}
    for n in (3, 7):
        frames = _frames(w, h, 1, n + 1)
        ref = gpu.Batch(p, n, reverse=True)
        _fill_pairs(gpu, ref, frames, w, h)
        ref.run()
        out[n] = (p, frames, levels(ref, p), levels(ref, p, "reverse"))
        ref.close()
    return out


# n = 3: ofdis_batch_run takes sub-batches of at least two frames, so 3 pairs run un-split under set_pipeline(2) and (3);
# n = 7 is cut into 2 and 3 ragged frame views, whose B planes must move with their A planes
@pytest.mark.parametrize("n", [3, 7])
@pytest.mark.parametrize("how,arg", [("pipeline", 2), ("pipeline", 3), ("graph", 1)])
def test_sequence_pipelined_and_graph(gpu, gray_ref, how, arg, n):
    p, frames, want_fw, want_rev = gray_ref[n]
    b = gpu.Batch(p, n, sequence=True, reverse=True)
    _fill_seq(gpu, b, frames, 256, 112)
    if how == "pipeline":
        b.set_pipeline(arg)
    else:
        b.set_graph(arg)
    for rep in range(2):
        b.run()
        if how == "pipeline":
            b.run()  # two passes in flight before anything joins
        check_levels(levels(b, p), want_fw, f"{how} {arg}, pass {rep}: forward")
        check_levels(levels(b, p, "reverse"), want_rev, f"{how} {arg}, pass {rep}: reverse")
        assert b.status() == 0
    b.close()


def test_sequence_warm_start(gpu, gray_ref):
    """set_initflow / set_initflow_reverse on a sequence context == the same warm start on a reverse context, pipelined too"""
    n = 7
    p, frames, cold_fw, _ = gray_ref[n]
    cw, ch = p.level_size(p.sc_f)
    rng = np.random.default_rng(78)
    init = [gpu.Dev((rng.standard_normal((n, ch // 2, cw // 2, 2)) * 0.7).astype(_f32)) for _ in range(2)]
    ref = gpu.Batch(p, n, reverse=True)
    _fill_pairs(gpu, ref, frames, 256, 112)
    b = gpu.Batch(p, n, sequence=True, reverse=True)
    _fill_seq(gpu, b, frames, 256, 112)
    b.set_pipeline(2)
    for c in (ref, b):
        c.set_initflow(init[0].ptr)
        c.set_initflow_reverse(init[1].ptr)
        c.run()
    want_fw = levels(ref, p)
    assert not np.array_equal(want_fw[p.sc_l], cold_fw[p.sc_l])
    check_levels(levels(b, p), want_fw, "warm start, forward")
    check_levels(levels(b, p, "reverse"), levels(ref, p, "reverse"), "warm start, reverse")
    ref.close()
    b.close()


# ------------------------------------------------------------------ 3. the input planes
@pytest.mark.parametrize("noc", [1, 3], ids=["gray", "rgb"])
def test_sequence_input_planes(gpu, noc):
    """Slot k of kinds 0..2 == the plain context's A planes of pair k; kinds 3..5 are kinds 0..2 one frame further on and
    equal the plain context's B planes -- B's gradients included, which a forward-only sequence context has too."""
    w, h, n = 256, 112, 3
    p = _params(2, w, h, noc)
    frames = _frames(w, h, noc, n + 1)
    ref = gpu.Batch(p, n, reverse=True)
    _fill_pairs(gpu, ref, frames, w, h)
    for reverse in (False, True):
        b = gpu.Batch(p, n, sequence=True, reverse=reverse)
        _fill_seq(gpu, b, frames, w, h)
        assert b.input_frames() == n + 1
        for l in range(p.sc_l, p.sc_f + 1):
            for j in range(3):
                assert b.input_ptr(l, 3 + j) == b.input_ptr(l, j) + 4 * b.input_elems(l), (l, j)
            assert not b.input_ptr(l, 6)
        for kind in range(6):
            want = _planes(gpu, ref, p, kind, n)
            got = _planes(gpu, b, p, kind, n)
            for l in want:
                assert_bits_equal(got[l], want[l], f"reverse={reverse}: input kind {kind}, level {l}")
        for j in range(3):  # the last slot: B of the last pair
            last = _planes(gpu, b, p, j, n + 1)
            want = _planes(gpu, ref, p, 3 + j, n)
            for l in want:
                assert_bits_equal(last[l][n], want[l][n - 1], f"slot {n} of kind {j}, level {l}")
        b.close()
    assert ref.input_frames() == n
    ref.close()


# ------------------------------------------------------------------ 4. pitched input
def _embed(frames, pitch, stride, offset, fill):
    """the frames' rows at offset + f * stride + y * pitch of a byte buffer otherwise full of `fill`"""
    n, h = frames.shape[:2]
    rows = frames.reshape(n, h, -1)
    buf = np.full(offset + n * stride + 64, fill, np.uint8)
    for f in range(n):
        for y in range(h):
            o = offset + f * stride + y * pitch
            buf[o:o + rows.shape[2]] = rows[f, y]
    return buf


# (noc, width, pitch, frame stride, byte offset of the first frame; 0 = packed)
PITCH_CASES = [
    pytest.param(1, 250, 256, 256 * (112 + 5), 0, id="gray-w250-pitch256-rows-between-frames"),
    pytest.param(1, 256, 512, 512 * 112 * 3 // 2, 0, id="gray-nv12-luma-pitch512"),      # the 16-byte streaming kernel
    pytest.param(1, 256, 0, 0, 4, id="gray-packed-base-offset-4"),                        # ... which this one must refuse
    pytest.param(1, 256, 272, 272 * 112 + 16, 0, id="gray-pitch272-streaming"),
    pytest.param(1, 256, 260, 260 * 112 + 4, 0, id="gray-pitch260-words"),
    pytest.param(1, 256, 258, 258 * 112 + 1, 0, id="gray-pitch258-bytes"),
    pytest.param(3, 256, 800, 800 * 112, 0, id="rgb-pitch800"),
]


@pytest.mark.parametrize("noc,w,pitch,stride,offset", PITCH_CASES)
def test_sequence_pitched_frames(gpu, noc, w, pitch, stride, offset):
    """Frames embedded in a larger buffer give the planes of the packed call, bit for bit, whatever the padding holds (it is
    never read)."""
    h, n = 112, 2
    p = _params(2, w, h, noc)
    frames = _frames(w, h, noc, n + 1)
    b = gpu.Batch(p, n, sequence=True)
    _fill_seq(gpu, b, frames, w, h)
    want = [_planes(gpu, b, p, kind, n + 1) for kind in range(3)]
    row = w * noc
    for fill in (0xAA, 0x17):
        buf = _embed(frames, pitch or row, stride or row * h, offset, fill)
        d = gpu.Dev(buf)
        for l in range(p.sc_l, p.sc_f + 1):  # nothing of the packed call may survive
            for kind in range(3):
                gpu.check(gpu.lib().ofdis_memcpy_h2d(b.input_ptr(l, kind), np.zeros_like(want[kind][l]).ctypes.data,
                                                     want[kind][l].nbytes))
        b.build_pyramids_u8_seq(d.ptr + offset, w, h, row_pitch=pitch, frame_stride=stride)
        _sync(gpu)
        for kind in range(3):
            got = _planes(gpu, b, p, kind, n + 1)
            for l in got:
                assert_bits_equal(got[l], want[kind][l], f"padding {fill:#x}: kind {kind}, level {l}")
        d.free()
    b.close()


# ------------------------------------------------------------------ 5. finish calls
def test_sequence_finish_calls(gpu, gray_ref):
    """upsample_bidir, the encoded upsample and interpolate of a sequence + reverse context == the reverse context's."""
    n, w, h = 3, 256, 112
    p, frames, _, _ = gray_ref[n]
    ref = gpu.Batch(p, n, reverse=True)
    da, db = gpu.Dev(frames[:-1]), gpu.Dev(frames[1:])
    ref.build_pyramids_u8(da.ptr, db.ptr, w, h)
    b = gpu.Batch(p, n, sequence=True, reverse=True)
    d = gpu.Dev(frames)
    b.build_pyramids_u8_seq(d.ptr, w, h)
    for c in (ref, b):
        c.run()
    names = ("forward flow", "reverse flow", "forward mask", "reverse mask")
    for got, want, name in zip(b.upsample_bidir(w, h), ref.upsample_bidir(w, h), names):
        assert_bits_equal(got, want, f"upsample_bidir: {name}")
    enc = gpu.Encoding(gpu.ENC_U8, 255.0 / 40.0, 127.5)
    got, want = b.upsample_frames_enc(0, n, w, h, enc), ref.upsample_frames_enc(0, n, w, h, enc)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert len(np.unique(want)) > 8
    times = (0.0, 0.5, 1.0)
    want = ref.interpolate(da.ptr, db.ptr, w, h, times)
    got = b.interpolate(d.ptr, d.ptr + w * h, w, h, times)  # img_b = frames + one frame
    assert np.array_equal(got, want)
    assert np.array_equal(got[:, 0], frames[:-1]) and np.array_equal(got[:, 2], frames[1:])
    got = b.interpolate(d.ptr, d.ptr + w * h, w, h, times, first=1, count=2)
    assert np.array_equal(got, want[1:])
    for c in (ref, b):
        c.close()


# ------------------------------------------------------------------ 6. rejections
def test_sequence_rejections(gpu):
    w, h, n = 256, 112, 2
    p = _params(2, w, h)
    L = gpu.lib()
    frames = _frames(w, h, 1, n + 1)
    d = gpu.Dev(frames)
    pyr = _host_pyramids(p, frames[:1])[0]
    n_lv = p.sc_f + 1
    keep = [[gpu._f(x) if x is not None else None for x in pl] for pl in pyr]  # (the pointer arrays borrow these)
    arr = [gpu._ptr_array(pl, n_lv) for pl in keep]
    seq, plain = gpu.Batch(p, n, sequence=True), gpu.Batch(p, n)
    assert L.ofdis_batch_build_pyramids_u8(seq.h, d.ptr, d.ptr + w * h, w, h, None) == -1
    assert "ofdis_batch_build_pyramids_u8_seq" in L.ofdis_last_error().decode()
    assert L.ofdis_batch_upload(seq.h, 0, arr[0], arr[1], arr[2], arr[0], None) == -1
    assert "ofdis_batch_upload_frame" in L.ofdis_last_error().decode()
    assert L.ofdis_batch_upload_b_gradients(seq.h, 0, arr[1], arr[2], None) == -1
    assert "ofdis_batch_upload_frame" in L.ofdis_last_error().decode()
    assert L.ofdis_batch_build_pyramids_u8_seq(plain.h, d.ptr, 0, 0, w, h, None) == -1
    assert L.ofdis_batch_upload_frame(plain.h, 0, arr[0], arr[1], arr[2], None) == -1
    assert L.ofdis_batch_build_pyramids_u8_seq(seq.h, d.ptr, w - 1, 0, w, h, None) == -1
    assert "row_pitch" in L.ofdis_last_error().decode()
    assert L.ofdis_batch_build_pyramids_u8_seq(seq.h, d.ptr, w, w * h - 1, w, h, None) == -1
    assert "frame_stride" in L.ofdis_last_error().decode()
    assert L.ofdis_batch_build_pyramids_u8_seq(seq.h, d.ptr, 0, 0, w - 40, h, None) == -1   # not the padding of this size
    assert L.ofdis_batch_build_pyramids_u8_seq(seq.h, None, 0, 0, w, h, None) == -1
    assert L.ofdis_batch_upload_frame(seq.h, n + 1, arr[0], arr[1], arr[2], None) == -1     # slots are 0 .. n
    assert L.ofdis_batch_upload_frame(seq.h, -1, arr[0], arr[1], arr[2], None) == -1
    assert L.ofdis_batch_upload_frame(seq.h, n, arr[0], arr[1], arr[2], None) == 0
    _sync(gpu)
    seq.close()
    plain.close()


# ------------------------------------------------------------------ 7. memory
def test_sequence_memory(gpu):
    """A clip needs three planes per frame and level where a reverse context holds six per pair."""
    w, h, n = 256, 112, 64
    p = _params(2, w, h)
    seq, rev = gpu.Batch(p, n, sequence=True, reverse=True), gpu.Batch(p, n, reverse=True)
    plane_floats = sum(seq.input_elems(l) for l in range(p.sc_l, p.sc_f + 1))
    assert plane_floats == sum((p.level_size(l)[0] + 2 * p.imgpadding) * (p.level_size(l)[1] + 2 * p.imgpadding)
                               for l in range(p.sc_l, p.sc_f + 1))
    print(f"device bytes at n = {n}: sequence + reverse {seq.device_bytes()}, reverse {rev.device_bytes()}")
    assert seq.device_bytes() < rev.device_bytes()
    assert rev.device_bytes() - seq.device_bytes() == (6 * n - 3 * (n + 1)) * plane_floats * 4
    assert seq.input_frames() == n + 1 and rev.input_frames() == n
    fwd_seq, fwd = gpu.Batch(p, n, sequence=True), gpu.Batch(p, n)
    assert fwd.device_bytes() - fwd_seq.device_bytes() == (4 * n - 3 * (n + 1)) * plane_floats * 4
    for b in (seq, rev, fwd_seq, fwd):
        b.close()
