"""GPU: ofdis_segment_overlap, _link, _chain, _relabel and _tracks (of_dis_amd/csrc/ofdis_segment_tracks.hip) against the
definitions of of_dis_amd/segments.py, every output compared bit for bit; the slots a definition leaves alone carry a pattern on
both sides.  Every condition on a generated input is checked on the model, never on the kernel.  The geometry the cases aim at:
a wavefront owns 64 consecutive pixels of a row, the overlap is accumulated in LDS up to 128 segment slots and in global memory
above, a workgroup of the LDS route owns a band of SEGTRACK_BAND_ROWS rows, and the per-pixel kernels grid-stride beyond
SEGTRACK_GRID_BLOCKS (SEGTRACK_LDS_GRID_BLOCKS) workgroups."""
import functools

import numpy as np
import pytest

from of_dis_amd import capi, segments as S
from seq_products import assert_same_bits, run_context

pytestmark = pytest.mark.gpu
_f32 = np.float32
LDS = capi.SEGTRACK_LDS_MAX_SEGMENTS


def _fill(shape, dtype, salt=0):
    """the pattern the untouched slots must keep: odd, so never a zero the call might have written"""
    n = int(np.prod(shape))
    return ((np.arange(n, dtype=np.int64) * 2654435761 + 12345 + salt) | 1).astype(dtype).reshape(shape)


def _info(counts):
    """info as ofdis_label_segments writes it, with info[:, 2] = counts and other numbers around it"""
    info = np.empty((len(counts), 4), np.int64)
    info[:, 0], info[:, 1], info[:, 3] = 1 << 40, -7, 123456789
    info[:, 2] = counts
    return info


# ------------------------------------------------------------------ overlap alone
def _wild_flow(rng, nmaps, h, w):
    """flows of a few pixels with NaN (one with a payload), infinities, +-4096 and the floats just beyond, 1e30 and +-x.5
    halves, which round to even"""
    flow = (rng.standard_normal((nmaps, h, w, 2)) * 3).astype(_f32)
    above = np.nextafter(_f32(4096.0), _f32(np.inf))
    pick = rng.random((nmaps, h, w, 2))
    for lo, value in ((0.00, np.nan), (0.02, np.inf), (0.04, -np.inf), (0.06, 4096.0), (0.08, -4096.0), (0.10, above),
                      (0.12, -above), (0.14, 1e30), (0.16, np.array([0xFFC00001], np.uint32).view(_f32)[0]),
                      (0.18, 0.5), (0.22, -0.5), (0.26, 1.5), (0.30, -1.5), (0.34, 2.5), (0.38, -2.5), (0.42, 3.5)):
        flow[(pick >= lo) & (pick < lo + (0.02 if lo < 0.18 else 0.04))] = value
    return flow


@functools.lru_cache(maxsize=None)
def _random_case(w, h, s, nmaps=3):
    """maps of values in -3 .. S + 3, info[:, 2] = S, S - 1, S + 5, wild flows: (segments, flow, info), read-only"""
    rng = np.random.default_rng(100000 * s + 10 * w + h)
    seg = rng.integers(-3, s + 4, (nmaps, h, w)).astype(np.int32)
    flow = _wild_flow(rng, nmaps, h, w)
    info = _info([(s, s - 1, s + 5)[k % 3] for k in range(nmaps)])
    for a in (seg, flow, info):
        a.setflags(write=False)
    return seg, flow, info


def _check_overlap(gpu, seg, flow, info, s, what):
    fill = _fill((len(seg) - 1, s, s), np.int32)
    want = S.segment_overlap_ref(seg, flow, info, s, overlap_fill=fill)
    assert_same_bits(gpu.segment_overlap(seg, flow, info, s, overlap_fill=fill), want, f"{what}: overlap")
    return want, fill


# one wavefront and less, 63 / 64 / 65 and 129 columns (one, two, three chunks per row, the last one short), several workgroups
# and three bands of rows (300x70), and the index extremes 8192x2 (where a flow of +-4096 stays inside) and 2x8192 (256 bands)
SIZES = [(1, 1), (63, 5), (64, 16), (65, 7), (129, 3), (300, 70), (8192, 2), (2, 8192)]
SEGMENTS = [1, 4, LDS, LDS + 1, 1024]   # both routes, on both sides of their boundary


@pytest.mark.parametrize("s", SEGMENTS)
@pytest.mark.parametrize("w,h", SIZES)
def test_overlap(gpu, w, h, s):
    seg, flow, info = _random_case(w, h, s)
    want, fill = _check_overlap(gpu, seg, flow, info, s, f"{w}x{h} S {s}")
    n = S.recorded_counts(info, s)
    assert n.tolist() == [s, s - 1, s]
    assert (want[0, :, s - 1:] == fill[0, :, s - 1:]).all() and (want[1, s - 1:] == fill[1, s - 1:]).all()   # beyond n: untouched
    if w * h >= 64 * 16 and 4 <= s <= LDS + 1:
        assert (want[:, :s - 1, :s - 1] > 0).any()


def test_the_wild_flows_hold_what_they_claim():
    """(on the inputs and the model alone) every special value is among the flows of recorded pixels, and at 8192x2 a flow of
    +-4096 lands inside the frame and is counted"""
    seg, flow, info = _random_case(300, 70, 4)
    u = flow[:2].reshape(-1)
    above = np.nextafter(_f32(4096.0), _f32(np.inf))
    for value in (np.inf, -np.inf, 4096.0, -4096.0, above, -above, 1e30, 0.5, -0.5, 1.5, 2.5, -2.5, 3.5):
        assert (u == _f32(value)).any(), value
    assert len(set(u[np.isnan(u)].view(np.uint32).tolist())) >= 2
    seg, flow, info = _random_case(8192, 2, 4)
    a, u, v = seg[0], flow[0, ..., 0], flow[0, ..., 1]
    far = (a >= 1) & (a <= 4) & (np.abs(u) == 4096) & (np.abs(v) < 0.4)
    xt = np.arange(8192)[None, :] + np.where(far, u, 0).astype(np.int64)
    hit = far & (xt >= 0) & (xt < 8192)
    b = seg[1][np.nonzero(hit)[0], xt[hit]]
    assert hit.any() and ((b >= 1) & (b <= 3)).any()


def test_overlap_with_64_distinct_keys_in_a_wavefront(gpu):
    """S = 1024, 64x16, no motion: every chunk of map 0 holds 64 different recorded values, so its wavefront issues 64 atomics"""
    rng = np.random.default_rng(64)
    seg = np.stack([np.stack([rng.permutation(1024)[:64] + 1 for y in range(16)]), rng.integers(1, 1025, (16, 64))]).astype(np.int32)
    flow = np.zeros((2, 16, 64, 2), _f32)
    assert all(len(set(row.tolist())) == 64 for row in seg[0]) and seg.min() >= 1 and seg.max() <= 1024
    want, _ = _check_overlap(gpu, seg, flow, _info([1024, 1024]), 1024, "64 keys")
    assert want[0].sum() == 64 * 16 and want[0].max() <= 16


@pytest.mark.parametrize("s", [1, LDS, LDS + 1])
def test_overlap_of_single_value_maps(gpu, s):
    """all 64 lanes of every wavefront share one key: one atomic per chunk, all on the same word"""
    seg = np.full((3, 70, 300), s, np.int32)
    flow = np.zeros((3, 70, 300, 2), _f32)
    flow[1, ..., 0] = 1.0   # pair 1: the last column leaves the frame
    want, _ = _check_overlap(gpu, seg, flow, _info([s, s, s]), s, "single value")
    assert want[0, s - 1, s - 1] == 300 * 70 and want[1, s - 1, s - 1] == 299 * 70


@pytest.mark.parametrize("s", [4, LDS + 1])
def test_later_grid_stride_trips(gpu, s):
    """Enough maps of 300x70 for a second trip of the loops that stride by the grid.  S = 129, the global route: 350 chunks per
    map, four per workgroup, so the chunk loops of strk_overlap_global_kernel and strk_relabel_kernel pass SEGTRACK_GRID_BLOCKS
    workgroups.  S = 4, the LDS route: three bands per pair, one per workgroup and trip, so the band loop of
    strk_overlap_lds_kernel passes SEGTRACK_LDS_GRID_BLOCKS (and the relabel loop its own cap by far)."""
    w, h = 300, 70
    chunks = h * -(-w // 64)
    if s > LDS:
        nmaps = -(-capi.SEGTRACK_GRID_BLOCKS * 4 // chunks) + 2
        assert (nmaps - 1) * chunks > 4 * capi.SEGTRACK_GRID_BLOCKS + chunks
    else:
        bands = -(-h // capi.SEGTRACK_BAND_ROWS)
        nmaps = -(-capi.SEGTRACK_LDS_GRID_BLOCKS // bands) + 2
        assert (nmaps - 1) * bands > capi.SEGTRACK_LDS_GRID_BLOCKS + bands
    assert nmaps * chunks > 4 * capi.SEGTRACK_GRID_BLOCKS
    rng = np.random.default_rng(s)
    seg = rng.integers(-1, s + 2, (nmaps, h, w)).astype(np.int32)
    flow = np.rint(rng.standard_normal((nmaps, h, w, 2)) * 4).astype(_f32) / 2   # halves and whole numbers
    info = _info(rng.integers(s - 1, s + 1, nmaps))
    want, _ = _check_overlap(gpu, seg, flow, info, s, f"{nmaps} maps")
    assert want[-1, :s - 1, :s - 1].sum() > 1000 and want[0, :s - 1, :s - 1].sum() > 1000   # the last pair is of the second trip
    ids = rng.integers(1, 1 << 20, (nmaps, s)).astype(np.int32)
    fill = _fill(seg.shape, np.int32)
    assert_same_bits(gpu.segment_relabel(seg, ids, info, s, track_map_fill=fill), S.segment_relabel_ref(seg, ids, info, s), "relabel")


# ------------------------------------------------------------------ link, chain and relabel on a clip of moving rectangles
CW, CH, CN = 130, 70, 6   # three chunks per row, the last of two pixels


@functools.lru_cache(maxsize=None)
def _rectangle_clip():
    """(label uint8 [6, 70, 130], flow float32 [6, 70, 130, 2]): rectangles in uniform motion, drawn at their rounded positions,
    each pixel carrying its rectangle's velocity.
      A 12x8, 4 px per map: exact, crosses x = 64; no speck is put beside it
      B 10x6, (2.5, 0.5) per map: crosses x = 64, overlaps itself only in part
      C 10x6, (3.5, 0) per map: leaves the frame on the right
      D  8x8, (2, 1) per map: born at map 2
      E  6x6, (0.5, 0) per map: dies after map 2
      F, G 8x6, (2, 0) and (-2, 0): touch at map 4 and are one component from then on
      T two pixels of map 0 that land on two separate pixels of map 1: a tie
    and 1 % of single-pixel specks without motion."""
    rng = np.random.default_rng(2026)
    fg = rng.random((CN, CH, CW)) < 0.01
    flow = np.zeros((CN, CH, CW, 2), _f32)
    rects = [("A", 40, 4, 12, 8, 4.0, 0.0, 0, 5), ("B", 50, 20, 10, 6, 2.5, 0.5, 0, 5), ("C", 118, 35, 10, 6, 3.5, 0.0, 0, 5),
             ("D", 10, 40, 8, 8, 2.0, 1.0, 2, 5), ("E", 90, 50, 6, 6, 0.5, 0.0, 0, 2), ("F", 20, 13, 8, 6, 2.0, 0.0, 0, 5),
             ("G", 44, 13, 8, 6, -2.0, 0.0, 0, 5)]
    for k in range(CN):
        for name, x0, y0, bw, bh, vx, vy, first, last in rects:
            if not first <= k <= last:
                continue
            x, y = int(np.rint(x0 + vx * (k - first))), int(np.rint(y0 + vy * (k - first)))
            if name == "A":
                fg[k, max(y - 1, 0):y + bh + 1, max(x - 1, 0):x + bw + 1] = False
            fg[k, y:y + bh, max(x, 0):x + bw] = True
            flow[k, y:y + bh, max(x, 0):x + bw] = (vx, vy)
    fg[0:2, 0:3, 0:6] = False
    fg[0, 1, 1:3] = True
    flow[0, 1, 2] = (1.0, 0.0)
    fg[1, 1, 1] = fg[1, 1, 3] = True
    label = np.where(fg, np.uint8(1), np.uint8(0))
    label.setflags(write=False)
    flow.setflags(write=False)
    return label, flow


@functools.lru_cache(maxsize=None)
def _labelled_clip(s, min_area):
    """the clip's (segments, records, info) by the model of ofdis_label_segments, conn 8; the record slots beyond n_k hold a
    pattern, which no later step may read"""
    label, flow = _rectangle_clip()
    out = S.label_segments_ref(label, flow, codes=2, conn=8, min_area=min_area, max_segments=s, records_fill=_fill((CN, s, 12), np.int64, 5))
    for a in out:
        a.setflags(write=False)
    return out


def _pair_facts(overlap, link, records, info, s, min_share):
    """what the model's link step met: (ties, bests that are not mutual, mutual bests the share test rejects)"""
    n, area = S.recorded_counts(info, s), S.segment_areas(records, s)
    ties = unmutual = unshared = 0
    for k in range(len(n) - 1):
        c = overlap[k, :n[k], :n[k + 1]].astype(np.int64)
        if not c.size:
            continue
        ties += int(((c == c.max(axis=1, keepdims=True)) & (c > 0)).sum(axis=1).max() > 1)
        ties += int(((c == c.max(axis=0, keepdims=True)) & (c > 0)).sum(axis=0).max() > 1)
        for a in range(n[k]):
            b = int(c[a].argmax())
            if c[a, b] > 0 and int(c[:, b].argmax()) != a:
                unmutual += 1
            elif c[a, b] > 0 and link[k, a] == 0:
                assert c[a, b] * 100 < min_share * min(area[k, a], area[k + 1, b])
                unshared += 1
    return ties, unmutual, unshared


CLIP_PARAMS = [(64, 0, 100), (64, 4, 90), (16, 0, 0)]   # S, min_area, min_share


@functools.lru_cache(maxsize=None)
def _clip_model(s, min_area, min_share):
    seg, rec, info = _labelled_clip(s, min_area)
    flow = _rectangle_clip()[1]
    overlap = S.segment_overlap_ref(seg, flow, info, s, overlap_fill=_fill((CN - 1, s, s), np.int32, 1))
    link = S.segment_link_ref(overlap, rec, info, s, min_share, link_fill=_fill((CN - 1, s), np.int32, 2))
    return overlap, link


def test_the_clip_holds_what_it_claims():
    """(on the model alone) over the parameter sets: a tie, a best that is not mutual, a share rejection, a track through all
    six maps, and a track born after map 0 that goes on"""
    facts = np.zeros(3, np.int64)
    full = later = 0
    for s, min_area, min_share in CLIP_PARAMS:
        seg, rec, info = _labelled_clip(s, min_area)
        overlap, link = _clip_model(s, min_area, min_share)
        facts += _pair_facts(overlap, link, rec, info, s, min_share)
        ids, tracks, tinfo = S.segment_chain_ref(link, rec, info, s, CN * s)
        t = tracks[:tinfo[1]]
        full += int((t[:, 2] == CN).sum())
        later += int(((t[:, 0] > 0) & (t[:, 2] > 1)).sum())
        print(f"S {s} min_area {min_area} min_share {min_share}: n_k {S.recorded_counts(info, s).tolist()} tinfo {tinfo.tolist()}")
        if (s, min_area) == (64, 4):   # the specks are gone: the rectangles, the tie's pieces apart
            assert S.recorded_counts(info, s).max() <= 12
            assert tinfo[3] == CN and ((t[:, 0] == 2) & (t[:, 2] == 4)).any()   # A all the way, D from map 2 to the end
    print("ties, not mutual, share rejections:", facts.tolist(), "tracks of length 6:", full, "born later and longer than 1:", later)
    assert (facts > 0).all() and full >= 1 and later >= 1


@pytest.mark.parametrize("s,min_area,min_share", CLIP_PARAMS)
def test_link_chain_and_relabel(gpu, s, min_area, min_share):
    """each step on the model's output of the step before, so that a step is compared on inputs that hold the fill pattern
    wherever the definition leaves them alone"""
    seg, rec, info = _labelled_clip(s, min_area)
    flow = _rectangle_clip()[1]
    overlap, link = _clip_model(s, min_area, min_share)
    assert_same_bits(gpu.segment_overlap(seg, flow, info, s, overlap_fill=_fill((CN - 1, s, s), np.int32, 1)), overlap, "overlap")
    assert_same_bits(gpu.segment_link(overlap, rec, info, s, min_share, link_fill=_fill((CN - 1, s), np.int32, 2)), link, "link")
    ntracks = int(S.segment_chain_ref(link, rec, info, s, 1)[2][0])
    assert ntracks > 3
    for max_tracks in (CN * s, ntracks, ntracks - 1, 1):
        fills = dict(ids_fill=_fill((CN, s), np.int32, 3), tracks_fill=_fill((max_tracks, 12), np.int64, 4))
        want = S.segment_chain_ref(link, rec, info, s, max_tracks, **fills)
        assert want[2][0] == ntracks and want[2][1] == min(ntracks, max_tracks)
        for g, w_, name in zip(gpu.segment_chain(link, rec, info, s, max_tracks, **fills), want, ("ids", "tracks", "tinfo")):
            assert_same_bits(g, w_, f"max_tracks {max_tracks}: {name}")
    ids = want[0]
    assert_same_bits(gpu.segment_relabel(seg, ids, info, s, track_map_fill=_fill(seg.shape, np.int32, 6)),
                     S.segment_relabel_ref(seg, ids, info, s), "relabel")


def test_chain_takes_any_link_array(gpu):
    """values out of range, several a for one b (no link step gives that): the smallest a is the predecessor; garbage records wrap"""
    rng = np.random.default_rng(11)
    s, nmaps = 300, 9
    link = rng.integers(-2, s + 3, (nmaps - 1, s)).astype(np.int32)
    rec = rng.integers(-(1 << 62), 1 << 62, (nmaps, s, 12))
    info = _info(rng.integers(s - 40, s + 10, nmaps))
    fills = dict(ids_fill=_fill((nmaps, s), np.int32, 3), tracks_fill=_fill((nmaps * s, 12), np.int64, 4))
    want = S.segment_chain_ref(link, rec, info, s, nmaps * s, **fills)
    assert 2 < want[2][3] and s < want[2][0] < nmaps * s
    for g, w_, name in zip(gpu.segment_chain(link, rec, info, s, nmaps * s, **fills), want, ("ids", "tracks", "tinfo")):
        assert_same_bits(g, w_, name)


def test_link_on_random_counts_with_many_ties(gpu):
    """S = 1024 and 200: small counts, so rows and columns are full of equal maxima; areas around the counts, so the share test cuts"""
    for s, nmaps in ((1024, 2), (200, 4)):
        rng = np.random.default_rng(s)
        overlap = (rng.integers(0, 4, (nmaps - 1, s, s)) * (rng.random((nmaps - 1, s, s)) < 0.02)).astype(np.int32)
        rec = rng.integers(-3, 9, (nmaps, s, 12))
        info = _info([s - 3] * nmaps)
        fill = _fill((nmaps - 1, s), np.int32, 2)
        want = S.segment_link_ref(overlap, rec, info, s, 60, link_fill=fill)
        assert 0 < (want[:, :s - 3] > 0).sum() < (nmaps - 1) * (s - 3) // 2
        assert_same_bits(gpu.segment_link(overlap, rec, info, s, 60, link_fill=fill), want, f"S {s}: link")


# ------------------------------------------------------------------ the composite
def _composite(gpu, seg, flow, rec, info, s, min_share, max_tracks, track_map=True):
    fills = dict(ids_fill=_fill((len(seg), s), np.int32, 3), tracks_fill=_fill((max_tracks, 12), np.int64, 4))
    got = gpu.segment_tracks(seg, flow, rec, info, s, min_share, max_tracks, track_map=track_map,
                             track_map_fill=_fill(seg.shape, np.int32, 6), **fills)
    want = S.segment_tracks_ref(seg, flow, rec, info, s, min_share, max_tracks, track_map=track_map, **fills)
    for g, w_, name in zip(got[:3], want[:3], ("ids", "tracks", "tinfo")):
        assert_same_bits(g, w_, f"composite: {name}")
    if track_map:
        assert_same_bits(got[3], want[3], "composite: track_map")
    else:
        assert got[3] is None
    return got


@pytest.mark.parametrize("s,min_area,min_share", CLIP_PARAMS)
def test_the_composite_is_the_four_calls(gpu, s, min_area, min_share):
    seg, rec, info = _labelled_clip(s, min_area)
    flow = _rectangle_clip()[1]
    max_tracks = 40
    first = _composite(gpu, seg, flow, rec, info, s, min_share, max_tracks)
    second = _composite(gpu, seg, flow, rec, info, s, min_share, max_tracks)
    without = _composite(gpu, seg, flow, rec, info, s, min_share, max_tracks, track_map=False)
    overlap = gpu.segment_overlap(seg, flow, info, s)
    link = gpu.segment_link(overlap, rec, info, s, min_share)
    fills = dict(ids_fill=_fill((CN, s), np.int32, 3), tracks_fill=_fill((max_tracks, 12), np.int64, 4))
    ids, tracks, tinfo = gpu.segment_chain(link, rec, info, s, max_tracks, **fills)
    four = (ids, tracks, tinfo, gpu.segment_relabel(seg, ids, info, s))
    for name, a, b, c, d in zip(("ids", "tracks", "tinfo", "track_map"), first, second, four, without):
        assert_same_bits(a, b, f"twice: {name}")
        assert_same_bits(a, c, f"four calls: {name}")
        if d is not None:
            assert_same_bits(a, d, f"without track_map: {name}")


def test_one_map(gpu):
    """N = 1: no pair, every recorded segment a track of length 1; the four calls take a clip of one map as well"""
    seg, rec, info = (a[:1] for a in _labelled_clip(64, 4))
    flow = _rectangle_clip()[1][:1]
    ids, tracks, tinfo, tmap = _composite(gpu, seg, flow, rec, info, 64, 50, 40)
    n = int(info[0, 2])
    assert n >= 5 and tinfo.tolist() == [n, n, 0, 1] and ids[0, :n].tolist() == list(range(1, n + 1))
    assert gpu.segment_overlap(seg, flow, info, 64).shape == (0, 64, 64)
    assert gpu.segment_link(np.zeros((0, 64, 64), np.int32), rec, info, 64, 50).shape == (0, 64)
    fills = dict(ids_fill=_fill((1, 64), np.int32, 3), tracks_fill=_fill((40, 12), np.int64, 4))   # (those of _composite)
    for g, w_, name in zip(gpu.segment_chain(np.zeros((0, 64), np.int32), rec, info, 64, 40, **fills), (ids, tracks, tinfo),
                           ("ids", "tracks", "tinfo")):
        assert_same_bits(g, w_, f"chain, one map: {name}")
    assert_same_bits(gpu.segment_relabel(seg, ids, info, 64), tmap, "relabel, one map")


# ------------------------------------------------------------------ end to end
def _moving_square_clip(w, h, nframes, side=40, small=14):
    """a textured background panning 2 px per frame, a differently textured square moving 3 px per frame against it, and a
    small one moving down on its own: the object to follow and the one for min_area to remove"""
    import gen_synth
    back = np.clip(np.rint(gen_synth._texture(np.random.default_rng(41), h, w)), 0, 255).astype(np.uint8)
    front = np.clip(np.rint(gen_synth._texture(np.random.default_rng(42), side, side)), 0, 255).astype(np.uint8)
    M = gen_synth.MARGIN
    clip = np.empty((nframes, h, w), np.uint8)
    for k in range(nframes):
        clip[k] = back[M:M + h, M + 2 * k:M + 2 * k + w]
        x, y = w // 2 - 3 * k, h // 3 + k
        clip[k, y:y + side, x:x + side] = front[M:M + side, M:M + side]
        clip[k, 16 + 3 * k:16 + 3 * k + small, 40:40 + small] = front[M:M + small, M + side - small:M + side]
    return clip


def test_end_to_end_moving_square(gpu):
    """sequence context -> global_motion -> motion_compensate -> label_segments -> segment_tracks with the context's own
    full-resolution flow: equal to the model on those real maps, records and flows, and on the model the large square is one
    track through all four pairs"""
    w, h, n = 256, 112, 4
    b, devs = run_context(gpu, _moving_square_clip(w, h, n + 1), "seq")
    try:
        flow = b.upsample(w, h)
        models, stats = b.global_motion(w, h, rounds=3, thresh=1.0)
        residual, label = b.motion_compensate(models, w, h, thresh=1.0)
    finally:
        b.close()
    assert flow.shape == (n, h, w, 2) and label.shape == (n, h, w)
    seg, rec, info = gpu.label_segments(label, residual, codes=S.SEG_MOVING, conn=8, min_area=500, max_segments=64)
    ids, tracks, tinfo, tmap = _composite(gpu, seg, flow, rec, info, 64, 50, 32)
    print("end to end: n_k", info[:, 2].tolist(), "tinfo", tinfo.tolist(), "tracks", tracks[:tinfo[1], :5].tolist())
    want = S.segment_tracks_ref(seg, flow, rec, info, 64, 50, 32)
    assert (info[:, 2] >= 1).all()
    largest = [int(rec[k, :info[k, 2], 0].argmax()) for k in range(n)]   # the square: the largest segment of every pair
    assert len({int(want[0][k, largest[k]]) for k in range(n)}) == 1
    t = int(want[0][0, largest[0]])
    assert want[1][t - 1, 0] == 0 and want[1][t - 1, 2] == n and want[2][3] == n
