"""-m gpu: track selection (include/ofdis.h: ofdis_track_select) against of_dis_amd/tracking.py (track_select_ref: the header's
definition in numpy), every comparison by bytes: codes and counts as integers, tracks and shapes as fp32 bits.

The slots come from the population of tests/test_track_select_ref.py, whose properties (every code occurs, a fair share is
kept, len 0 and 1 occur) are asserted there on the model.  Every device array holds idle slots filled with 0xAB behind the
slots in use and a guard behind its end; what the call may not write must still hold 0xAB afterwards.  No code, count, slot
number or track entry of the model is 0xAB.., so a kept fill is an unwritten entry."""
import functools

import numpy as np
import pytest

from of_dis_amd import capi, tracking
from of_dis_amd.tracking import TrackSelectParams, track_select_ref
from test_track_select_ref import POPULATIONS, SIZE, population

pytestmark = pytest.mark.gpu
_f32 = np.float32
GUARD = 4096
FILL8, FILL32 = 0xAB, 0xABABABAB
SPARE = 9                                  # idle slots behind the slots in use
LANES = capi.TRACK_SELECT_LANES
SECOND_TRIP = LANES * LANES + 1            # the smallest count whose scan takes a second trip: LANES + 1 workgroup records


def _models(pop, which):
    return {"none": None, "translation": pop[3], "affine": pop[4]}[which]


def _slots(n, lmax):
    """the first n slots of the population that holds them"""
    tracks, start, length = population(max(n, 200) if n != SECOND_TRIP else SECOND_TRIP, lmax)[:3]
    return tracks[:, :n], start[:n], length[:n]


@functools.lru_cache(maxsize=None)
def _want(n, lmax, which, params_key=None, max_out=None):
    """the model's outputs, computed once per case and shared (nobody writes to them)"""
    pop = population(max(n, 200) if n != SECOND_TRIP else SECOND_TRIP, lmax)
    params = TrackSelectParams(*params_key) if params_key else None
    out = track_select_ref(*_slots(n, lmax), _models(pop, which), SIZE, params, max_out)
    for a in out:
        a.setflags(write=False)
    return out


def _key(t):
    return (t.min_len, float(t.min_std), float(t.max_std), float(t.max_step), float(t.max_step_share), float(t.min_camera), t.tests)


def _filled(a, spare):
    """the array with `spare` more slots of 0xAB along its slot axis (the last but one of tracks, the only one otherwise)"""
    axis = a.ndim - 2 if a.ndim > 1 else 0
    shape = list(a.shape)
    shape[axis] = spare
    return np.concatenate([a, np.full(shape, FILL32, np.uint32).view(a.dtype)], axis=axis)


class _Run:
    """One call on guarded device arrays.  `src` = (tracks, start, length) fills the first slots of max_tracks, the rest is
    0xAB; info[0] = n_info; every output, optional ones included unless `optional` is False, holds 0xAB before the call."""

    def __init__(self, gpu, src, n_info, max_tracks, models=None, params=None, max_out=None, stream=None, optional=True):
        tracks, start, length = src
        lmax = tracks.shape[0] - 1
        max_out = max_tracks if max_out is None else max_out
        spare = max_tracks - tracks.shape[1]
        self.inputs = dict(tracks=_filled(tracks.view(np.uint32), spare), start=_filled(start, spare), len=_filled(length, spare),
                           info=np.array([n_info, 7], np.int64))
        if models is not None:
            self.inputs["models"] = np.ascontiguousarray(models)
        self.din = {k: gpu.Dev(v) for k, v in self.inputs.items()}
        wb = gpu.track_select_work_bytes(max_tracks)
        assert wb == 64 * -(-max_tracks // LANES)
        self.sizes = dict(code=max_tracks, counts=56, tracks_out=(lmax + 1) * max_out * 8, start_out=max_out * 4, len_out=max_out * 4,
                          info_out=16, index=max_out * 4, shape_out=max_out * lmax * 8, work=wb)
        self.dev = {k: gpu.Dev(np.full(v + GUARD, FILL8, np.uint8)) for k, v in self.sizes.items()}
        d, opt = self.dev, (lambda k: self.dev[k].ptr if optional else None)
        gpu.track_select_dev(self.din["tracks"].ptr, self.din["start"].ptr, self.din["len"].ptr, self.din["info"].ptr, lmax,
                             max_tracks, max_out, d["tracks_out"].ptr, d["start_out"].ptr, d["len_out"].ptr, d["info_out"].ptr,
                             d["work"].ptr, wb, self.din["models"].ptr if models is not None else None,
                             len(models) if models is not None else 0, SIZE[0], SIZE[1], params, opt("code"), opt("counts"),
                             opt("index"), opt("shape_out"), stream.ptr if stream else None)
        gpu.check(gpu.lib().ofdis_sync(stream.ptr if stream else None))
        raw = {k: d[k].get((v + GUARD,), np.uint8) for k, v in self.sizes.items()}
        for k, v in self.sizes.items():
            assert (raw[k][v:] == FILL8).all(), f"guard behind {k}"
        for k, v in self.inputs.items():   # the inputs are inputs
            assert np.array_equal(self.din[k].get(v.shape, v.dtype).view(np.uint8), v.view(np.uint8)), f"input {k} changed"
        cut = lambda k, dtype, shape: raw[k][:self.sizes[k]].view(dtype).reshape(shape)
        self.code, self.counts = cut("code", np.uint8, (max_tracks,)), cut("counts", np.int64, (7,))
        self.tracks_out = cut("tracks_out", np.uint32, (lmax + 1, max_out, 2))
        self.start_out, self.len_out = cut("start_out", np.int32, (max_out,)), cut("len_out", np.int32, (max_out,))
        self.info_out, self.index = cut("info_out", np.int64, (2,)), cut("index", np.int32, (max_out,))
        self.shape_out = cut("shape_out", np.uint32, (max_out, lmax, 2))
        self.optional = optional

    def check(self, want, n, what, nan_payload=True):
        """against the model's outputs `want` of the first n input slots, and nothing written beyond what they allow"""
        code, counts, tracks_out, start_out, len_out, info, index, shape = want
        k = int(info[0])
        assert list(self.info_out) == list(info), (what, self.info_out, info)
        if self.optional:
            assert np.array_equal(self.code[:n], code), (what, np.flatnonzero(self.code[:n] != code)[:8])
            assert (self.code[n:] == FILL8).all(), what
            assert np.array_equal(self.counts, counts), (what, self.counts, counts)
            assert np.array_equal(self.index[:k], index), what
            got, ref = self.shape_out[:k], shape.view(np.uint32)
            if not nan_payload:   # (positions that are not finite were kept: the header leaves a NaN's payload open)
                assert np.array_equal(np.isnan(got.view(_f32)), np.isnan(shape)), what
                got, ref = np.where(np.isnan(shape), 0, got), np.where(np.isnan(shape), 0, ref)
            if not np.array_equal(got, ref):
                bad = np.argwhere(got != ref)
                r, j, c = bad[0]
                raise AssertionError(f"{what}: {len(bad)} of {got.size} shape values differ; first at output slot {r} (input slot "
                                     f"{index[r]}), step {j}, component {c}: {got.view(_f32)[r, j, c]!r} vs {shape[r, j, c]!r}")
        else:
            for name in ("code", "counts", "index", "shape_out"):
                assert (getattr(self, name).view(np.uint8) == FILL8).all(), (what, name)
        assert np.array_equal(self.tracks_out[:, :k], tracks_out.view(np.uint32)), what
        assert np.array_equal(self.start_out[:k], start_out) and np.array_equal(self.len_out[:k], len_out), what
        # nothing at or above nkept_written
        assert (self.tracks_out[:, k:] == FILL32).all() and (self.start_out[k:].view(np.uint32) == FILL32).all(), what
        assert (self.len_out[k:].view(np.uint32) == FILL32).all(), what
        if self.optional:
            assert (self.index[k:].view(np.uint32) == FILL32).all() and (self.shape_out[k:] == FILL32).all(), what


def test_the_second_trip_of_the_scan_is_what_the_largest_case_reaches():
    """the constant the sizes below rest on, tied to the library by the work buffer's size (tests/test_track_select_abi.py)"""
    assert SECOND_TRIP == 65537 and (SECOND_TRIP, 2) in POPULATIONS
    assert capi.track_select_work_bytes(SECOND_TRIP) == 64 * (LANES + 1) and capi.track_select_work_bytes(SECOND_TRIP - 1) == 64 * LANES


# ------------------------------------------------------------------ 1. against the definition
CASES = [(n, lmax) for lmax in (1, 2, 15) for n in (1, 17, 200)] + [(SECOND_TRIP, 2)]


@pytest.mark.parametrize("which", ["none", "translation", "affine"])
@pytest.mark.parametrize("n,lmax", CASES, ids=[f"n{n}-L{lmax}" for n, lmax in CASES])
def test_select_matches_the_definition(gpu, n, lmax, which):
    pop = population(max(n, 200) if n != SECOND_TRIP else SECOND_TRIP, lmax)
    want = _want(n, lmax, which)
    print(f"n {n} lmax {lmax} models {which}: " + ", ".join(f"{k} {c}" for k, c in zip(tracking.TS_NAMES, want[1])))
    run = _Run(gpu, _slots(n, lmax), n, n + SPARE, _models(pop, which))
    run.check(want, n, f"n {n} lmax {lmax} {which}")
    assert run.counts.sum() == n and run.counts[0] == run.info_out[0]


def test_on_a_stream_of_the_callers(gpu):
    pop = population(200, 15)
    stream = gpu.Stream()
    try:
        _Run(gpu, _slots(200, 15), 200, 200 + SPARE, pop[4], stream=stream).check(_want(200, 15, "affine"), 200, "non-null stream")
    finally:
        stream.close()


def test_other_thresholds(gpu):
    """every parameter away from its default, min_len among them; infinite upper limits"""
    pop = population(200, 15)
    for t in (TrackSelectParams(min_len=9, min_std=3.0, max_std=40.0, max_step=25.0, max_step_share=0.5, min_camera=0.25),
              TrackSelectParams(max_std=np.inf, max_step=np.inf), TrackSelectParams(min_std=0.0, max_step_share=0.0, min_camera=0.0),
              TrackSelectParams(max_std=0.0, max_step=0.0, max_step_share=1.0)):
        want = _want(200, 15, "affine", _key(t))
        assert len(np.unique(want[0])) >= 3, want[1]
        _Run(gpu, _slots(200, 15), 200, 200 + SPARE, pop[4], t).check(want, 200, repr(t))


def test_the_optional_outputs_left_out(gpu):
    pop = population(200, 2)
    _Run(gpu, _slots(200, 2), 200, 200 + SPARE, pop[3], optional=False).check(_want(200, 2, "translation"), 200, "optional NULL")


# ------------------------------------------------------------------ 2. edges
@pytest.mark.parametrize("n,lmax", [(200, 15), (SECOND_TRIP, 2)])
def test_everything_rejected(gpu, n, lmax):
    t = TrackSelectParams(min_len=lmax + 2)
    want = _want(n, lmax, "none", _key(t))
    assert list(want[5]) == [0, 0] and want[1][tracking.TS_SHORT] == n
    run = _Run(gpu, _slots(n, lmax), n, n + SPARE, None, t)
    run.check(want, n, "everything rejected")
    for name in ("tracks_out", "start_out", "len_out", "index", "shape_out"):   # no output slot is written
        assert (getattr(run, name).view(np.uint8) == FILL8).all(), name


@pytest.mark.parametrize("n,lmax,which", [(200, 15, "affine"), (200, 1, "none"), (SECOND_TRIP, 2, "translation")])
def test_everything_kept_with_all_tests_off(gpu, n, lmax, which):
    pop = population(n, lmax)
    src = _slots(n, lmax)
    t = TrackSelectParams(tests=0)
    run = _Run(gpu, src, n, n + SPARE, _models(pop, which), t)
    run.check(_want(n, lmax, which, _key(t)), n, "everything kept", nan_payload=False)
    # the outputs equal the inputs bit for bit, NaN tails included, and index is the identity
    assert list(run.info_out) == [n, 0] and list(run.counts) == [n, 0, 0, 0, 0, 0, 0] and not run.code[:n].any()
    assert np.array_equal(run.tracks_out[:, :n], src[0].view(np.uint32))
    assert (run.tracks_out[:, :n] == tracking.ENDED_BITS).any()
    assert np.array_equal(run.start_out[:n], src[1]) and np.array_equal(run.len_out[:n], src[2])
    assert np.array_equal(run.index[:n], np.arange(n))


@pytest.mark.parametrize("n,lmax,room", [(200, 15, None), (200, 15, 1), (17, 1, 2), (SECOND_TRIP, 2, None), (SECOND_TRIP, 2, LANES + 3)])
def test_an_output_set_smaller_than_the_kept_slots(gpu, n, lmax, room):
    pop = population(max(n, 200), lmax)
    nkept = int(_want(n, lmax, "affine")[1][0])
    room = nkept // 3 if room is None else room
    assert 1 <= room < nkept
    want = _want(n, lmax, "affine", None, room)
    assert list(want[5]) == [room, nkept - room]
    run = _Run(gpu, _slots(n, lmax), n, n + SPARE, pop[4], max_out=room)
    run.check(want, n, f"room {room} of {nkept}")   # (the guards stand right behind slot room - 1)
    # exactly as many slots as there are kept ones: nothing dropped
    _Run(gpu, _slots(n, lmax), n, n + SPARE, pop[4], max_out=nkept).check(_want(n, lmax, "affine", None, nkept), n, "exact room")


def test_lengths_zero_and_one_occur(gpu):
    """on the model: the cases above ran slots with len 0 (short) and len 1 (static, or kept with the tests off)"""
    for lmax in (1, 2, 15):
        length = _slots(200, lmax)[2]
        code = _want(200, lmax, "none")[0]
        assert (length == 0).any() and (length == 1).any()
        assert (code[length == 0] == tracking.TS_SHORT).all() and (code[length == 1] == tracking.TS_STATIC).any()
        assert np.isin(code[length == 1], (tracking.TS_STATIC, tracking.TS_INVALID)).all()   # (a single position may be a NaN)


def test_ntracks_is_read_on_the_device(gpu):
    """info[0] decides how many slots are looked at, not the arrays' size: fewer than the slots that hold tracks, and (clamped to
    max_tracks) more than there are"""
    pop = population(200, 15)
    src = _slots(200, 15)
    _Run(gpu, src, 17, 200 + SPARE, pop[4]).check(_want(17, 15, "affine"), 17, "info[0] = 17 of 200 filled slots")
    _Run(gpu, src, 0, 200 + SPARE, pop[4]).check(track_select_ref(*_slots(0, 15), pop[4], SIZE), 0, "info[0] = 0")
    _Run(gpu, src, 200 + 1000, 200, pop[4]).check(_want(200, 15, "affine"), 200, "info[0] above max_tracks")
    _Run(gpu, src, -5, 200, pop[4]).check(track_select_ref(*_slots(0, 15), pop[4], SIZE), 0, "info[0] negative")


# ------------------------------------------------------------------ 3. composition: the selected set is a drop-in
def test_descriptors_and_bof_of_the_selected_set(gpu):
    """ofdis_track_select -> ofdis_track_descriptors -> ofdis_track_bof, device to device, on the tracks of
    tests/test_gpu_descriptors.py: rows `index` of the same calls on the original set"""
    from test_gpu_descriptors import CASES as DESC_CASES, MIN_FLOW, _case, assert_descriptors_equal
    case = DESC_CASES[0]
    w, h, _, _, npairs, _, N, nxy, nt = case
    frames, fw, (tracks, start, length, info), want_desc, _ = _case(*case, 1)
    n, lmax = len(length), tracks.shape[0] - 1
    layout = tracking.descriptor_layout(N, nxy, nt)
    D = layout["dims"]
    t = TrackSelectParams(min_len=3, min_std=0.8)
    want = track_select_ref(tracks, start, length, params=t)
    index, k = want[6], int(want[5][0])
    assert n // 5 < k < 4 * n // 5 and len(np.unique(want[0])) >= 3, want[1]
    original = gpu.track_descriptors(frames, fw, tracks, start, length, N, nxy, nt, MIN_FLOW)
    assert_descriptors_equal(original, want_desc, "the original set")

    max_tracks, room = n + SPARE, k + SPARE
    run = _Run(gpu, (tracks, start, length), n, max_tracks, None, t, max_out=room)
    run.check(want, n, "the descriptor tracks")
    assert np.array_equal(run.shape_out[:k], original[1][index].view(np.uint32))   # shape_out is that call's shape

    dfr, dfw = gpu.Dev(frames), gpu.Dev(fw)
    dh, dsh = gpu.Dev(np.full(room * D * 4, FILL8, np.uint8)), gpu.Dev(np.full(room * lmax * 8, FILL8, np.uint8))
    d = run.dev
    gpu.track_descriptors_dev(dfr.ptr, dfw.ptr, npairs, w, h, 1, d["tracks_out"].ptr, d["start_out"].ptr, d["len_out"].ptr,
                              d["info_out"].ptr, lmax, room, N, nxy, nt, MIN_FLOW, dh.ptr, dsh.ptr)
    desc = tracking.normalize_descriptors_u8(want_desc[0], layout)
    codebook = np.ascontiguousarray(np.concatenate([desc[index][::9], desc[3::40]]))
    min_len = lmax + 1
    db, dw = gpu.Dev(np.full(16 * len(codebook), FILL8, np.uint8)), gpu.Dev(np.full(room * 16, FILL8, np.uint8))
    dc = gpu.Dev(codebook)
    gpu.track_bof_dev(dh.ptr, d["len_out"].ptr, d["info_out"].ptr, room, nxy, nt, dc.ptr, len(codebook), min_len, db.ptr, dw.ptr)
    gpu.check(gpu.lib().ofdis_sync(None))
    hist = dh.get((room, D), np.uint32)
    shape = dsh.get((room, lmax, 2), _f32)
    assert_descriptors_equal((hist[:k], shape[:k]), (original[0][index], original[1][index]), "the selected set")
    assert (hist[k:] == FILL32).all() and (shape[k:].view(np.uint32) == FILL32).all()
    words = tracking.codebook_assign_ref(desc[index], layout, codebook)[0]
    assert np.array_equal(dw.get((room, 4), np.int32)[:k], words)
    want_bof = tracking.bof_ref(words, length[index], len(codebook), min_len)
    assert want_bof.sum() > 0 and np.array_equal(db.get((4, len(codebook)), np.uint32), want_bof)
    # ... which differs from the bag of the original set: the selection did something
    assert not np.array_equal(want_bof, tracking.bof_ref(tracking.codebook_assign_ref(desc, layout, codebook)[0], length, len(codebook), min_len))


def test_select_on_host_arrays(gpu):
    """capi.track_select: the same outputs cut to nkept_written, an empty set included"""
    pop = population(200, 15)
    got = gpu.track_select(*_slots(200, 15), pop[4], SIZE)
    for g, w_ in zip(got, _want(200, 15, "affine")):
        assert g.dtype == w_.dtype and g.shape == w_.shape and np.array_equal(g.view(np.uint8), w_.view(np.uint8))
    got = gpu.track_select(*_slots(200, 15), max_out=5, shape=False)
    assert got[7] is None and list(got[5]) == [5, _want(200, 15, "none")[1][0] - 5]
    assert np.array_equal(got[6], _want(200, 15, "none")[6][:5])
    empty = gpu.track_select(*_slots(0, 15))
    assert list(empty[5]) == [0, 0] and empty[2].shape == (16, 0, 2) and not empty[1].any()


# ------------------------------------------------------------------ 4. the command-line tool
def test_flow_images_track_select(gpu, tmp_path):
    """tools/flow_images.py --sequence --reverse --dense-tracks ... --track-select SPEC --global-motion --descriptors ...: the
    track and descriptor files hold the kept tracks of the run without --track-select, <stem>_dcode.npy and _dindex.npy say
    which; without --dense-tracks it is refused"""
    import os
    import subprocess
    import sys
    from PIL import Image
    from seq_products import smooth_clip
    from test_gpu_dense_tracks import STRIDE, WINDOW, _clip_threshold
    w, h, n = 250, 107, 3
    frames = smooth_clip(w, h, 1, n + 1)
    T = _clip_threshold(frames, STRIDE, WINDOW)
    paths = []
    for k, f in enumerate(frames):
        paths.append(str(tmp_path / f"f{k}.png"))
        Image.fromarray(f).save(paths[-1])
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "flow_images.py")
    run = lambda args: subprocess.run([sys.executable, tool] + args, capture_output=True, text=True, timeout=300)
    common = ["--sequence", "--reverse", "--dense-tracks", f"5:2:{T}:3", "--descriptors", "16:2:3:0.4"]
    files = ("dtracks", "dstart", "dlen", "dhist", "dshape")
    load = lambda stem, names: [np.load(f"{stem}_{name}.npy") for name in names]
    res = run(common + paths + [str(tmp_path / "all")])
    assert res.returncode == 0, (res.stdout, res.stderr)
    res = run(common + ["--track-select", "2:0.3:50:20:0.7:0.25", "--global-motion"] + paths + [str(tmp_path / "sel")])
    assert res.returncode == 0, (res.stdout, res.stderr)
    everything, kept = load(tmp_path / "all", files), load(tmp_path / "sel", files)
    code, index = load(tmp_path / "sel", ("dcode", "dindex"))
    assert code.dtype == np.uint8 and index.dtype == np.int32 and code.shape == everything[2].shape
    assert np.array_equal(index, np.flatnonzero(code == 0)) and 0 < len(index) < len(code)
    assert np.array_equal(kept[0].view(np.uint32), everything[0][:, index].view(np.uint32))
    for got, full in zip(kept[1:], everything[1:]):
        assert got.dtype == full.dtype and np.array_equal(got.view(np.uint8), np.ascontiguousarray(full[index]).view(np.uint8))
    # the camera models can only take kept tracks out: every other code is the one the model gives without them
    t = TrackSelectParams(2, 0.3, 50.0, 20.0, 0.7, 0.25)
    ref = track_select_ref(*everything[:3], params=t)[0]
    assert np.array_equal(code[ref != 0], ref[ref != 0]) and np.isin(code[ref == 0], (tracking.TS_KEPT, tracking.TS_CAMERA)).all()
    res = run(["--sequence", "--reverse", "--track-select"] + paths + [str(tmp_path / "none")])
    assert res.returncode != 0 and "--dense-tracks" in (res.stderr + res.stdout)
