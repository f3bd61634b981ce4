"""GPU: ofdis_label_segments (of_dis_amd/csrc/ofdis_segments.hip) against the definition, of_dis_amd/segments.py:
label_segments_ref -- segments, info and the whole records array (the slots the definition leaves alone carry a pattern on
both sides) compared bit for bit.  Every condition on a generated input is checked on the model, never on the kernel.  The
geometry the cases aim at: a wavefront owns 64 consecutive pixels of a row, the numbering counts blocks of 256 raster indices,
and every kernel grid-strides."""
import functools

import numpy as np
import pytest

import segments_hooks
from launch_hooks import launch_limits
from of_dis_amd import segments as S
from seq_products import assert_same_bits, run_context

pytestmark = pytest.mark.gpu
_f32 = np.float32
FG = 1            # the foreground byte of the generated maps; codes = 1 << FG
BACKGROUND = np.array([0, 2, 7, 8, 9, 255], np.uint8)   # what their other pixels hold: codes 0..7 not in `codes`, and bytes >= 8


def _fill(nmaps, max_segments):
    """the pattern the untouched record slots must keep"""
    return (np.arange(nmaps * max_segments * S.SEG_RECORD_FIELDS, dtype=np.int64) * 2654435761 + 12345).reshape(
        nmaps, max_segments, S.SEG_RECORD_FIELDS) | 1


def _as_label(fg, seed=0):
    """bool [..] -> uint8: FG where set, a mix of the other bytes elsewhere"""
    rng = np.random.default_rng(seed)
    return np.where(fg, np.uint8(FG), BACKGROUND[rng.integers(0, len(BACKGROUND), fg.shape)]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _random_maps(nmaps, w, h, densities, seed=0):
    rng = np.random.default_rng(1000 * w + 10 * h + nmaps + seed)
    fg = np.stack([rng.random((h, w)) < densities[m % len(densities)] for m in range(nmaps)])
    label = _as_label(fg, w + h)
    label.setflags(write=False)
    return label


@functools.lru_cache(maxsize=None)
def _random_flow(nmaps, w, h, wild):
    rng = np.random.default_rng(77 + w + h + nmaps)
    flow = (rng.standard_normal((nmaps, h, w, 2)) * 6).astype(_f32)
    if wild:
        above = np.nextafter(_f32(4096.0), _f32(np.inf))
        pick = rng.random((nmaps, h, w, 2))
        for lo, value in ((0.00, np.nan), (0.03, np.inf), (0.06, -np.inf), (0.09, 4096.0), (0.12, -4096.0), (0.15, above),
                          (0.18, -above), (0.21, 1e30), (0.24, np.array([0xFFC00001], np.uint32).view(_f32)[0]),
                          (0.27, 0.501953125), (0.30, -0.505859375)):
            flow[(pick >= lo) & (pick < lo + 0.03)] = value
    flow.setflags(write=False)
    return flow


def _check(gpu, label, flow=None, what="", run=None, **kw):
    """the device call and the model on the same arguments; returns the model's (segments, records, info)"""
    nmaps, h, w = label.shape
    kw.setdefault("codes", 1 << FG)
    kw.setdefault("max_segments", h * w)
    fill = _fill(nmaps, kw["max_segments"])
    want = S.label_segments_ref(label, flow, records_fill=fill, **kw)
    got = (run or gpu.label_segments)(label, flow, records_fill=fill, **kw)
    for g, w_, name in zip(got, want, ("segments", "records", "info")):
        assert_same_bits(g, w_, f"{what} {kw}: {name}")
    return want


# ------------------------------------------------------------------ sizes
# one wavefront and less, 63 / 64 / 65 and 129 columns (one, two, three chunks per row, the last one short), several workgroups
# (300x70), 255 / 256 / 257 raster indices (the blocks of the numbering), and the index extremes 8192x2 and 2x8192
SIZES = [(1, 1), (1, 9), (13, 1), (63, 5), (64, 16), (65, 7), (129, 3), (300, 70), (8192, 2), (2, 8192), (51, 5), (64, 4), (257, 1)]


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("w,h", SIZES)
def test_sizes(gpu, w, h, conn):
    _check(gpu, _random_maps(1, w, h, (0.5,)), conn=conn, what=f"{w}x{h}")
    want = _check(gpu, _random_maps(3, w, h, (0.1, 0.593, 0.9)), _random_flow(3, w, h, False), conn=conn, what=f"3 maps {w}x{h}")
    if w * h >= 64:
        assert (want[2][:, 0] >= 1).all()


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("density", [0.1, 0.5, 0.593, 0.9])
def test_random_maps(gpu, density, conn):
    want = _check(gpu, _random_maps(2, 300, 70, (density,), seed=3), _random_flow(2, 300, 70, False), conn=conn, what=f"density {density}")
    assert (want[2][:, 0] >= (2 if density < 0.9 else 1)).all()   # (at 0.9 the map is one component)


# ------------------------------------------------------------------ adversarial maps, 130x70: three chunks per row, the last of two pixels
AW, AH = 130, 70


def _serpentine():
    """a one-pixel-wide path filling the map: every other row is full, the rows between join them at alternating ends"""
    m = np.zeros((AH, AW), bool)
    m[0::2] = True
    m[1::4, AW - 1] = True
    m[3::4, 0] = True
    return m


def _comb():
    """vertical teeth that join only in the last row"""
    m = np.zeros((AH, AW), bool)
    m[:, 0::2] = True
    m[AH - 1] = True
    return m


def _spiral():
    m = np.zeros((AH, AW), bool)
    x0, y0, x1, y1 = 0, 0, AW - 1, AH - 1
    while x1 - x0 >= 2 and y1 - y0 >= 2:
        m[y0, x0:x1 + 1] = m[y0:y1 + 1, x1] = m[y1, x0 + 2:x1 + 1] = m[y0 + 2:y1 + 1, x0 + 2] = True
        x0, y0, x1, y1 = x0 + 2, y0 + 2, x1 - 2, y1 - 2
        m[y0, x0] = True   # the way in to the next turn
    return m


def _checkerboard():
    y, x = np.mgrid[0:AH, 0:AW]
    return (x + y) % 2 == 0


def _diagonal_touches():
    """blobs that touch only by a corner: across the chunk boundary at x = 64 in both directions, at the map's last chunk
    (x = 128), and onto a blob whose root is the first index of a block of 256 (index 256 is x = 126 of row 1)"""
    m = np.zeros((AH, AW), bool)
    m[2:5, 60:64] = m[5:8, 64:68] = True        # down-right across x = 64
    m[12:15, 64:68] = m[15:18, 60:64] = True    # down-left across x = 64
    m[22:25, 124:128] = m[25:28, 128:130] = True
    m[0, 120:126] = m[1, 126:130] = True
    m[40, 63] = m[41, 64] = m[42, 63] = m[43, 64] = True   # a zigzag of single pixels on the boundary
    return m


ADVERSARIAL = {"serpentine": _serpentine, "comb": _comb, "spiral": _spiral, "checkerboard": _checkerboard,
               "diagonal touches": _diagonal_touches, "all foreground": lambda: np.ones((AH, AW), bool),
               "all background": lambda: np.zeros((AH, AW), bool)}
# what the model must find in them: name -> {conn: ncomp}
ADVERSARIAL_NCOMP = {"serpentine": {4: 1, 8: 1}, "comb": {4: 1, 8: 1}, "spiral": {4: 1, 8: 1},
                     "checkerboard": {4: AW * AH // 2, 8: 1}, "diagonal touches": {4: 12, 8: 5},
                     "all foreground": {4: 1, 8: 1}, "all background": {4: 0, 8: 0}}


@pytest.mark.parametrize("conn", [4, 8])
def test_adversarial_maps(gpu, conn):
    """one call over all of them: maps never interact"""
    names = list(ADVERSARIAL)
    label = _as_label(np.stack([ADVERSARIAL[n]() for n in names]), 4)
    seg, rec, info = _check(gpu, label, _random_flow(len(names), AW, AH, False), conn=conn, what="adversarial")
    for m, name in enumerate(names):
        assert info[m, 0] == ADVERSARIAL_NCOMP[name][conn], (name, info[m])
    none = names.index("all background")
    assert not seg[none].any() and info[none].tolist() == [0, 0, 0, 0]
    assert (rec[none] == _fill(len(names), AW * AH)[none]).all()   # no record touched


def test_the_adversarial_paths_are_what_they_claim():
    """(on the model alone) the serpentine is one pixel wide and a single path; the comb's teeth are apart above the last row"""
    s = _serpentine()
    assert S.label_segments_ref(_as_label(s), codes=2, conn=8, max_segments=1)[2][0, 0] == 1
    assert not (s[1::2].sum(axis=1) != 1).any()
    c = _comb()
    assert S.label_segments_ref(_as_label(c[:-1]), codes=2, conn=8, max_segments=1)[2][0, 0] == AW // 2
    assert S.label_segments_ref(_as_label(_spiral()), codes=2, conn=4, max_segments=1)[2][0, 3] > AW * AH // 3


# ------------------------------------------------------------------ filter and truncation
@pytest.mark.parametrize("conn", [4, 8])
def test_min_area_and_max_segments(gpu, conn):
    label = _random_maps(3, 130, 35, (0.45, 0.5, 0.3), seed=1)
    flow = _random_flow(3, 130, 35, True)
    seen = []
    for min_area in (0, 1, 2, 9, 130 * 35 + 1):
        seg, rec, info = _check(gpu, label, flow, conn=conn, min_area=min_area, what="min_area")
        seen.append(info[:, :2].copy())
    assert (seen[0] == seen[1]).all() and (seen[0][:, 0] == seen[0][:, 1]).all()   # max(min_area, 1)
    for both in (seen[2], seen[3]):   # components kept AND removed, in every map
        assert ((both[:, 1] >= 1) & (both[:, 1] < both[:, 0])).all(), both
    assert (seen[4][:, 1] == 0).all() and (seen[4][:, 0] > 0).all()
    nkept = int(seen[2][:, 1].min())
    assert nkept >= 3
    for max_segments in (1, nkept - 1):
        seg, rec, info = _check(gpu, label, flow, conn=conn, min_area=2, max_segments=max_segments, what="max_segments")
        assert (info[:, 2] == max_segments).all() and (info[:, 1] > max_segments).all()
        assert (seg.reshape(3, -1).max(axis=1) == info[:, 1]).all()   # numbered beyond the records
    # room to spare: the tail keeps the pattern (compared as part of the whole array; stated once here on the model's copy)
    seg, rec, info = _check(gpu, label, flow, conn=conn, min_area=2, max_segments=nkept + 700, what="tail")
    for m in range(3):
        assert (rec[m, info[m, 2]:] == _fill(3, nkept + 700)[m, info[m, 2]:]).all() and info[m, 2] < nkept + 700


# ------------------------------------------------------------------ optional outputs, flows, codes
def test_either_output_alone_and_flow_given_or_not(gpu):
    label, flow = _random_maps(3, 65, 7, (0.5,)), _random_flow(3, 65, 7, True)
    fill = _fill(3, 40)
    want = S.label_segments_ref(label, flow, codes=2, conn=8, min_area=2, max_segments=40, records_fill=fill)
    assert np.isin(want[1][0, :want[2][0, 2], 8], range(1, 60)).any() and (want[1][:, :4, 8] < want[1][:, :4, 0]).any()
    seg, none, info = gpu.label_segments(label, flow, codes=2, conn=8, min_area=2, max_segments=40, records=False)
    assert none is None
    assert_same_bits(seg, want[0], "records = NULL: segments")
    assert_same_bits(info, want[2], "records = NULL: info")
    none, rec, info = gpu.label_segments(label, flow, codes=2, conn=8, min_area=2, max_segments=40, segments=False, records_fill=fill)
    assert none is None
    assert_same_bits(rec, want[1], "segments = NULL: records")
    assert_same_bits(info, want[2], "segments = NULL: info")
    noflow = _check(gpu, label, None, conn=8, min_area=2, max_segments=40, what="flow = NULL")
    assert not noflow[1][0, :noflow[2][0, 2], 8:].any() and (noflow[1][..., :8] == want[1][..., :8]).all()


@pytest.mark.parametrize("conn", [4, 8])
def test_wild_flows(gpu, conn):
    """NaN (with payloads), infinities, +-4096 and the floats just beyond, values that round to even"""
    label, flow = _random_maps(2, 129, 11, (0.7,)), _random_flow(2, 129, 11, True)
    seg, rec, info = _check(gpu, label, flow, conn=conn, what="wild flows")
    big = rec[0, :info[0, 2]]
    assert ((big[:, 8] > 0) & (big[:, 8] < big[:, 0])).any() and np.isnan(flow).any() and np.isinf(flow).any()


def test_codes_select_the_bytes(gpu):
    rng = np.random.default_rng(8)
    label = rng.choice(np.array([0, 1, 2, 3, 7, 8, 64, 255], np.uint8), (2, 9, 70))
    for codes in (1, 1 << 7, (1 << 1) | (1 << 2), 0xFF):
        want = _check(gpu, label, codes=codes, conn=4, what=f"codes {codes:#x}")
        assert want[2][0, 3] == sum(int((label[0] == b).sum()) for b in range(8) if (codes >> b) & 1) > 0


# ------------------------------------------------------------------ independence and repeatability
def test_a_map_does_not_depend_on_its_neighbours(gpu):
    a, b = _random_maps(1, 130, 35, (0.55,), seed=5), _random_maps(1, 130, 35, (0.9,), seed=6)
    fa, fb = _random_flow(1, 130, 35, False), _random_flow(1, 130, 35, True)
    kw = dict(codes=2, conn=8, min_area=3, max_segments=64)
    one = gpu.label_segments(a, fa, records_fill=_fill(1, 64), **kw)
    three = gpu.label_segments(np.concatenate([a, b, a]), np.concatenate([fa, fb, fa]), records_fill=np.concatenate([_fill(1, 64)] * 3), **kw)
    for m in (0, 2):
        for x, y, name in zip(one, three, ("segments", "records", "info")):
            assert_same_bits(y[m], x[0], f"slot {m}: {name}")
    assert three[2][1].tolist() != three[2][0].tolist()


def test_the_same_call_twice_gives_the_same_bits(gpu):
    label, flow = _random_maps(3, 300, 70, (0.593, 0.5, 0.62), seed=9), _random_flow(3, 300, 70, True)
    kw = dict(codes=2, conn=4, min_area=2, max_segments=2000, records_fill=_fill(3, 2000))
    first, second = gpu.label_segments(label, flow, **kw), gpu.label_segments(label, flow, **kw)
    for x, y, name in zip(first, second, ("segments", "records", "info")):
        assert_same_bits(x, y, name)
    want = S.label_segments_ref(label, flow, **kw)
    assert (want[2][:, 1] < want[2][:, 0]).all() and (want[2][:, 1] < 2000).all()
    assert max(want[1][m, :want[2][m, 2], 0].max() for m in range(3)) > 500   # large tortuous components among them
    for x, y, name in zip(first, want, ("segments", "records", "info")):
        assert_same_bits(x, y, name)


# ------------------------------------------------------------------ launch limits
@pytest.mark.parametrize("conn", [4, 8])
def test_later_grid_stride_trips(gpu, conn):
    """GRID_MAX_BLOCKS lowered to 2 and to 3 workgroups in the test library: the chunk kernels make 130 and more trips at 300x70,
    the block kernels 125, the scan over the maps two"""
    assert segments_hooks.work_bytes(3, 300, 70) == gpu.lib().ofdis_segments_work_bytes(3, 300, 70) == S.segments_work_bytes(3, 300, 70)
    label, flow = _random_maps(3, 300, 70, (0.5, 0.593, 0.1), seed=2), _random_flow(3, 300, 70, True)
    for blocks in (2, 3):
        def run(label, flow, records_fill, codes, conn, min_area, max_segments):
            with launch_limits(grid_max_blocks=blocks):
                return segments_hooks.label_segments(gpu, label, flow, codes, conn, min_area, max_segments, records_fill)
        _check(gpu, label, flow, conn=conn, min_area=2, max_segments=300, run=run, what=f"{blocks} workgroups")


# ------------------------------------------------------------------ end to end
def _moving_square_clip(w, h, nframes, side=36, small=16):
    """a textured background panning 2 px per frame, a differently textured square moving 3 px per frame against it, and a
    small one moving down on its own: the object to keep and the one for min_area to remove"""
    import gen_synth
    back = np.clip(np.rint(gen_synth._texture(np.random.default_rng(31), h, w)), 0, 255).astype(np.uint8)
    front = np.clip(np.rint(gen_synth._texture(np.random.default_rng(32), side, side)), 0, 255).astype(np.uint8)
    M = gen_synth.MARGIN
    clip = np.empty((nframes, h, w), np.uint8)
    for k in range(nframes):
        clip[k] = back[M:M + h, M + 2 * k:M + 2 * k + w]
        x, y = w // 2 - 3 * k, h // 3 + k
        clip[k, y:y + side, x:x + side] = front[M:M + side, M:M + side]
        clip[k, 20 + 3 * k:20 + 3 * k + small, 40:40 + small] = front[M:M + small, M + side - small:M + side]
    return clip


def test_end_to_end_moving_square(gpu):
    """sequence context -> batch_global_motion -> batch_motion_compensate (label and residual) -> label_segments: equal to
    the model on those real labels and residuals.  How well the segment matches the square is the probe's figure
    (tools/segments_probe.py), not asserted here."""
    w, h, n = 256, 112, 2
    b, devs = run_context(gpu, _moving_square_clip(w, h, n + 1), "seq")
    try:
        models, stats = b.global_motion(w, h, rounds=3, thresh=1.0)
        residual, label = b.motion_compensate(models, w, h, thresh=1.0)
    finally:
        b.close()
    assert label.shape == (n, h, w) and residual.shape == (n, h, w, 2)
    seg, rec, info = _check(gpu, label, residual, codes=S.SEG_MOVING, conn=8, min_area=500, max_segments=64, what="end to end")
    print("end to end: info", info.tolist(), "largest areas", [int(rec[m, :info[m, 2], 0].max()) if info[m, 2] else 0 for m in range(n)])
    assert (info[:, 1] >= 1).all() and (info[:, 1] < info[:, 0]).all()   # on the model: kept and removed in every pair
