"""-m gpu: the bag-of-features encoding (include/ofdis.h: ofdis_descriptor_normalize, ofdis_codebook_assign, ofdis_bof_histogram,
ofdis_track_bof) against of_dis_amd/tracking.py (normalize_descriptors_u8, codebook_assign_ref, bof_ref), every comparison by
integer equality.

The hist arrays are synthetic (no flow run): 200 rows per descriptor size, the first ones holding the edge values; a case takes
the first ntracks rows and the first nwords words, so the model is computed once per size and codebook prefix and shared.  The
conditions on the inputs (ties, clamps, a used and an unused word) are checked on the model, never on the kernels."""
import functools

import numpy as np
import pytest

from of_dis_amd import tracking
from test_gpu_descriptors import CASES as DESC_CASES, MIN_FLOW, _case as _desc_case

pytestmark = pytest.mark.gpu
# (nxy, nt) with channels of 8/9, 96/108 and 1024/1152 entries, C = nxy^2 nt = 1, 12 and 128: 1, 2 and 16/18 k-steps.  That is
# bof_assign_kernel<2, 8> twice and <18, 1> at channels that are whole k-steps; <6, 3> is not among them (SWEEP_LAYOUTS)
LAYOUTS = [(1, 1), (2, 3), (4, 8)]
NWORDS = [1, 5, 16, 37, 300]         # below, at and above the 16 words of an MFMA; more than one staged tile of 16, 48 or 128
NTRACKS = [1, 15, 17, 200]           # below and above the 16 tracks of an MFMA; more than one workgroup at 64 slots
LMAX = 3
GUARD = 256
TOP = 2 ** 32 - 1

# One (nxy, nt) for each of the 28 values of C the public ranges (nxy 1 .. 4, nt 1 .. 8) give: everything behind the
# descriptors sees the layout through C alone.  Shared with tests/test_gpu_kmeans.py; tests/test_descriptor_layout_classes.py
# (CPU) derives every layout's class from the launchers' own choices -- the assignment kernel, the k-steps of both channel
# lengths and whether the last one and its last 16-byte fragment are cut, the lanes and passes of the k-means sum, 9 C mod 4,
# the finish kernel's thread split -- and holds this list, and the subsets below, to a member of every class that occurs.
# Behind each layout: C, and the seconds the numpy model took on one CPU core for its cases here (the six of
# test_the_calls_match_the_model_at_every_layout, 200 rows against 5, 16 TG + 1 and 32 TG + 13 words) and in
# tests/test_gpu_kmeans.py (its four of test_the_calls_match_the_model_at_every_layout), when the list was written.
SWEEP_LAYOUTS = [
    (1, 1),   # C 1: 0.06 + 0.01 s
    (1, 2),   # C 2: 0.04 + 0.01 s
    (1, 3),   # C 3: 0.06 + 0.01 s
    (1, 4),   # C 4: 0.06 + 0.01 s
    (1, 5),   # C 5: 0.08 + 0.01 s
    (1, 6),   # C 6: 0.09 + 0.01 s
    (1, 7),   # C 7: 0.11 + 0.02 s
    (2, 2),   # C 8: 0.11 + 0.01 s
    (3, 1),   # C 9: 0.15 + 0.02 s
    (2, 3),   # C 12: 0.18 + 0.02 s
    (4, 1),   # C 16: 0.10 + 0.03 s
    (3, 2),   # C 18: 0.11 + 0.03 s
    (2, 5),   # C 20: 0.14 + 0.03 s
    (2, 6),   # C 24: 0.14 + 0.04 s
    (3, 3),   # C 27: 0.17 + 0.04 s
    (2, 7),   # C 28: 0.18 + 0.05 s
    (2, 8),   # C 32: 0.19 + 0.06 s
    (3, 4),   # C 36: 0.24 + 0.06 s
    (3, 5),   # C 45: 0.14 + 0.07 s
    (4, 3),   # C 48: 0.14 + 0.07 s
    (3, 6),   # C 54: 0.16 + 0.10 s
    (3, 7),   # C 63: 0.18 + 0.11 s
    (4, 4),   # C 64: 0.19 + 0.10 s
    (3, 8),   # C 72: 0.19 + 0.12 s
    (4, 5),   # C 80: 0.23 + 0.13 s
    (4, 6),   # C 96: 0.28 + 0.17 s
    (4, 7),   # C 112: 0.30 + 0.22 s
    (4, 8),   # C 128: 0.37 + 0.23 s
]
NEW_LAYOUTS = [s for s in SWEEP_LAYOUTS if s not in LAYOUTS]   # the 25 that LAYOUTS' full parametrisation does not run
SWEEP_NTRACKS = [17, 200]
SWEEP_NWORDS = ["5", "tile+1", "2tile+13"]   # with tile = 16 TG words: a tile with idle words, a second tile of one word, a third
                                             # tile that ends inside a group of 16 -- 5, 49 and 109 for <6, 3>
# one layout per assignment kernel for a second workgroup whose last wavefronts are partly or wholly idle (64 TG + 23 tracks):
# <2, 8> with both k-steps, <6, 3> and <18, 1> with a cut last fragment
SECOND_WORKGROUP_LAYOUTS = [(2, 3), (3, 3), (3, 5)]
# <6, 3> and <18, 1> with a cut last fragment and k-step (C 27: 216/243 entries; C 45: 360/405), for the structured codebooks
STRUCTURED_LAYOUTS = [(3, 3), (3, 5)]
_id = lambda s: f"{s[0]}x{s[0]}x{s[1]}"


def _layout(nxy, nt):
    return tracking.descriptor_layout(12, nxy, nt)   # (12: a patch every nxy divides; the layout depends on nxy and nt alone)


def _nwords(size, which):
    """a codebook size of SWEEP_NWORDS for the layout's assignment kernel, its tile as the launcher's own choice gives it"""
    from launch_hooks import bof_shape
    tile = 16 * bof_shape(size[0] * size[0] * size[1])[2]
    return {"5": 5, "tile+1": tile + 1, "2tile+13": 2 * tile + 13}[which]


def _edge_rows(hist, layout, rng):
    """rows 1 .. 8 of `hist`: zero channels, clamped entries, entries near 2^32, one nonzero entry (row 0 stays ordinary:
    it is the only row of the cases with one track)"""
    segs = tracking._channel_slices(layout)
    hist[1, segs[1]] = 0                                        # a zero channel between ordinary ones
    hist[2] = 0                                                 # all zero
    hist[3] = rng.integers(0, 50, hist.shape[1])                # one dominant entry per channel: clamped
    for seg in segs:
        hist[3, seg.start + 3] = 100000
    hist[4] = rng.integers(TOP - 1000, TOP + 1, hist.shape[1])  # every entry near 2^32: the largest sums
    hist[5] = 0
    for seg, v in zip(segs, (1, TOP, 7, TOP - 1)):              # one nonzero entry per channel: 255
        hist[5, seg.stop - 1] = v
    hist[6] = rng.integers(0, 2 ** 32, hist.shape[1]) * (rng.random(hist.shape[1]) < 0.3)  # sparse and large
    hist[7, segs[0]] = 0
    hist[7, segs[3]] = 0
    hist[8] = 1                                                 # flat


def _codebook(desc, layout, rng, nwords):
    """words 0 and 1 equidistant from descriptor 0 in every channel (a tie: word 0), word 2 a copy of word 0 (never used),
    words 3 and 4 the corners 0 and 255, then other descriptors themselves with repeats, perturbed descriptors and noise"""
    n, D = desc.shape
    cb = np.zeros((nwords, D), np.uint8)
    step = lambda v: v + 2 if v < 128 else v - 2
    for k, at in ((0, 0), (1, 1)):
        cb[k] = desc[0]
        for seg in tracking._channel_slices(layout):
            cb[k, seg.start + at] = step(int(desc[0, seg.start + at]))
    cb[2] = cb[0]
    cb[3], cb[4] = 0, 255
    for k in range(5, nwords):
        kind = k % 4
        src = desc[1 + (k * 7) % (n - 1)]   # (never descriptor 0)
        if kind == 0:
            cb[k] = src
        elif kind == 1:
            cb[k] = cb[k - 1]                                   # a repeat of the word before: never used
        elif kind == 2:
            cb[k] = np.clip(src.astype(int) + rng.integers(-3, 4, D), 0, 255)
        else:
            cb[k] = rng.integers(0, 256, D)
    return cb


@functools.lru_cache(maxsize=None)
def _data(nxy, nt):
    """hist [200][D], len [200], the model's desc and the codebook of 300 words (nobody writes to them)"""
    layout = _layout(nxy, nt)
    rng = np.random.default_rng(1000 * nxy + nt)
    n, D = max(NTRACKS), layout["dims"]
    proto = rng.integers(0, 4000, (6, D))
    hist = (proto[rng.integers(0, 6, n)] * rng.integers(1, 300, (n, 1)) + rng.integers(0, 600, (n, D))).astype(np.uint32)
    hist[0] = rng.integers(0, 100000, D)   # (unlike every other row: only words 0 .. 2 come near it)
    _edge_rows(hist, layout, rng)
    length = rng.integers(1, LMAX + 2, n).astype(np.int32)
    length[0] = LMAX + 1
    desc = tracking.normalize_descriptors_u8(hist, layout)
    codebook = _codebook(desc, layout, rng, max(NWORDS))
    for a in (hist, length, desc, codebook):
        a.setflags(write=False)
    return layout, hist, length, desc, codebook


@functools.lru_cache(maxsize=None)
def _assigned(nxy, nt, nwords):
    """the model's (words, dist) of all 200 rows against the first nwords words, and which (row, channel) minima are ties for
    certain: the nearest word has a later copy in that channel (np.argmin took the first one)"""
    layout, _, _, desc, codebook = _data(nxy, nt)
    words, dist = tracking.codebook_assign_ref(desc, layout, codebook[:nwords])
    ties = np.zeros(words.shape, bool)
    for c, seg in enumerate(tracking._channel_slices(layout)):
        _, inverse, counts = np.unique(codebook[:nwords, seg], axis=0, return_inverse=True, return_counts=True)
        ties[:, c] = counts[inverse.ravel()][words[:, c]] > 1
    words.setflags(write=False), dist.setflags(write=False)
    return words, dist, ties


def _padded(a):
    """nine more slots behind the rows of `a`, every byte 0xAB"""
    row = int(np.prod(a.shape[1:], dtype=np.int64)) * a.itemsize
    return np.concatenate([a, np.frombuffer(b"\xab" * (9 * row), a.dtype).reshape((9,) + a.shape[1:])])


class _Run:
    """the four calls on the first ntracks rows with max_tracks = ntracks + 9 slots; every output pre-filled with 0xAB"""

    def __init__(self, gpu, nxy, nt, ntracks, nwords, min_len, dropped=0, stream=None, rows=None):
        layout, hist, length, _, codebook = _data(nxy, nt)
        if rows is not None:   # (hist, length) of more rows than _data has
            hist, length = rows
        assert ntracks <= len(hist) and nwords <= len(codebook)
        hist, length, codebook = hist[:ntracks], length[:ntracks], codebook[:nwords]
        self.n, self.nwords, self.D, self.slots = ntracks, nwords, layout["dims"], ntracks + 9
        self.gpu, self.args, self.stream = gpu, (nxy, nt), stream
        s = stream.ptr if stream else None
        self.dh, self.dl = gpu.Dev(_padded(hist)), gpu.Dev(_padded(length))
        self.di, self.dc = gpu.Dev(np.array([ntracks, dropped], np.int64)), gpu.Dev(codebook)
        self.sizes = dict(desc=self.slots * self.D, words=self.slots * 16, dist=self.slots * 16, bof=16 * nwords,
                          fwords=self.slots * 16, fbof=16 * nwords, nbof=16 * nwords)
        self.dev = {k: gpu.Dev(np.full(v + GUARD, 0xAB, np.uint8)) for k, v in self.sizes.items()}
        d, L = self.dev, gpu.lib()
        gpu.check(L.ofdis_descriptor_normalize(self.dh.ptr, self.di.ptr, self.slots, nxy, nt, d["desc"].ptr, s))
        gpu.check(L.ofdis_codebook_assign(d["desc"].ptr, self.di.ptr, self.slots, nxy, nt, self.dc.ptr, nwords, d["words"].ptr,
                                          d["dist"].ptr, s))
        gpu.check(L.ofdis_bof_histogram(d["words"].ptr, self.dl.ptr, self.di.ptr, self.slots, nwords, min_len, d["bof"].ptr, s))
        self.fused(min_len, "fbof", "fwords")
        self.fused(min_len, "nbof", None)
        self.raw = self.fetch()

    def fused(self, min_len, bof, words):
        nxy, nt = self.args
        self.gpu.track_bof_dev(self.dh.ptr, self.dl.ptr, self.di.ptr, self.slots, nxy, nt, self.dc.ptr, self.nwords, min_len,
                               self.dev[bof].ptr, self.dev[words].ptr if words else None, self.stream.ptr if self.stream else None)

    def fetch(self):
        self.gpu.check(self.gpu.lib().ofdis_sync(self.stream.ptr if self.stream else None))
        raw = {k: self.dev[k].get((v + GUARD,), np.uint8) for k, v in self.sizes.items()}
        for k, v in self.sizes.items():
            assert (raw[k][v:] == 0xAB).all(), f"guard behind {k}"
        return raw

    def rows(self, key, dtype, width):
        """(the slots below ntracks, the slots from ntracks on) of a per-slot output"""
        a = self.raw[key][:self.sizes[key]].view(dtype).reshape(self.slots, width)
        return a[:self.n], a[self.n:]

    def counts(self, key):
        return self.raw[key][:self.sizes[key]].view(np.uint32).reshape(4, self.nwords)


def _check(run, want_desc, want_words, want_dist, length, min_len, what):
    fillw = np.frombuffer(b"\xab" * 4, np.int32)[0]
    desc, idle = run.rows("desc", np.uint8, run.D)
    assert (idle == 0xAB).all(), what
    assert np.array_equal(desc, want_desc), (what, "desc", np.argwhere(desc != want_desc)[:3])
    for key, want in (("words", want_words), ("dist", want_dist), ("fwords", want_words)):
        got, idle = run.rows(key, np.int32, 4)
        assert (idle == fillw).all(), (what, key)
        assert np.array_equal(got, want), (what, key, np.argwhere(got != want)[:3], got[got != want][:3], want[got != want][:3])
    want_bof = tracking.bof_ref(want_words, length, run.nwords, min_len)
    assert (want_bof.sum(1) == (length >= min_len).sum()).all()
    for key in ("bof", "fbof", "nbof"):   # (no count is 0xABABABAB: a few hundred tracks)
        assert np.array_equal(run.counts(key), want_bof), (what, key)


# ------------------------------------------------------------------ 1. the calls against the model, the fused route against the chain
def _model_conditions(size, nwords, ntracks):
    """the conditions on the inputs of one case, asserted on the model: a tie resolved to the lower index, an unused word, entries
    0 and 255, a zero channel, hist near 2^32.  One word is used by every track and cannot be tied or unused"""
    nxy, nt = size
    layout, hist, length, desc, codebook = _data(nxy, nt)
    words, dist, ties = _assigned(nxy, nt, nwords)
    used = np.unique(words[:ntracks])
    assert len(used) >= 1
    if nwords > 1:
        assert ties[:ntracks].any() and len(used) < nwords, (ties[:ntracks].sum(), len(used))
        assert words[0].tolist() == [0] * 4 and dist[0].tolist() == [4] * 4   # the equidistant pair: the lower index
    if ntracks >= 15:
        assert (desc[:ntracks] == 255).any() and (desc[:ntracks] == 0).any() and (hist[:ntracks] >= TOP - 1000).any()
        assert not desc[2].any() and not desc[1, tracking._channel_slices(layout)[1]].any()
    assert dist.max() <= 1152 * 255 * 255
    return length, desc, words, dist


def _calls_match_the_model(gpu, size, nwords, ntracks):
    nxy, nt = size
    length, desc, words, dist = _model_conditions(size, nwords, ntracks)
    for min_len in (1, LMAX + 1):
        run = _Run(gpu, nxy, nt, ntracks, nwords, min_len, dropped=5 if ntracks == 17 else 0)
        _check(run, desc[:ntracks], words[:ntracks], dist[:ntracks], length[:ntracks], min_len, (size, nwords, ntracks, min_len))
        assert np.array_equal(run.di.get((2,), np.int64), [ntracks, 5 if ntracks == 17 else 0])   # the inputs are inputs


@pytest.mark.parametrize("ntracks", NTRACKS)
@pytest.mark.parametrize("nwords", NWORDS)
@pytest.mark.parametrize("size", LAYOUTS, ids=_id)
def test_the_calls_match_the_model(gpu, size, nwords, ntracks):
    _calls_match_the_model(gpu, size, nwords, ntracks)


@pytest.mark.parametrize("ntracks", SWEEP_NTRACKS)
@pytest.mark.parametrize("nwords", SWEEP_NWORDS)
@pytest.mark.parametrize("size", NEW_LAYOUTS, ids=_id)
def test_the_calls_match_the_model_at_every_layout(gpu, size, nwords, ntracks):
    """the other 25 values of C: normalize, assign, histogram and the fused route with and without words, guards, idle slots and
    both min_len, at codebook sizes chosen from the tile of the layout's own assignment kernel"""
    _calls_match_the_model(gpu, size, _nwords(size, nwords), ntracks)


@functools.lru_cache(maxsize=None)
def _more_rows(nxy, nt, ntracks):
    """(hist, length, desc) of ntracks rows: the 200 of _data over and over, the later copies moved a little"""
    layout, hist, length, _, _ = _data(nxy, nt)
    copy = np.arange(ntracks) // len(hist)
    at = np.arange(ntracks) % len(hist)
    hist = hist[at] ^ (copy[:, None] * (1 + np.arange(hist.shape[1]) % 7)).astype(np.uint32)   # (low bits: no entry leaves uint32)
    length = length[at]
    desc = tracking.normalize_descriptors_u8(hist, layout)
    for a in (hist, length, desc):
        a.setflags(write=False)
    return hist, length, desc


@pytest.mark.parametrize("size", SECOND_WORKGROUP_LAYOUTS, ids=_id)
def test_a_second_workgroup_with_idle_wavefronts(gpu, size):
    """64 TG + 23 tracks (+ 9 idle slots): the second workgroup of every assignment kernel holds one full group of 16 tracks, one
    of 7 live and 9 idle ones, and wavefronts with no track at all"""
    from launch_hooks import bof_shape
    nxy, nt = size
    tg = bof_shape(nxy * nxy * nt)[2]
    ntracks, nwords = 64 * tg + 23, _nwords(size, "2tile+13")
    layout, _, _, _, codebook = _data(nxy, nt)
    hist, length, desc = _more_rows(nxy, nt, ntracks)
    words, dist = tracking.codebook_assign_ref(desc, layout, codebook[:nwords])
    assert 64 * tg < ntracks and ntracks + 9 <= 2 * 64 * tg and len(np.unique(words // 16)) > 1   # two workgroups; words of more than one group of 16
    for min_len in (1, LMAX + 1):
        run = _Run(gpu, nxy, nt, ntracks, nwords, min_len, rows=(hist, length))
        _check(run, desc, words, dist, length, min_len, (size, ntracks, nwords, min_len))


# ------------------------------------------------------------------ 2. codebooks with structure, on descriptors given directly
def _assign(gpu, desc, codebook, nxy, nt):
    words, dist = gpu.codebook_assign(desc, codebook, nxy, nt)
    want = tracking.codebook_assign_ref(desc, _layout(nxy, nt), codebook)
    assert np.array_equal(words, want[0]) and np.array_equal(dist, want[1]), (np.argwhere(words != want[0])[:3],
                                                                              np.argwhere(dist != want[1])[:3])
    return words, dist


@pytest.mark.parametrize("size", LAYOUTS + STRUCTURED_LAYOUTS, ids=_id)
def test_a_codebook_drawn_from_the_descriptors(gpu, size):
    nxy, nt = size
    _, _, _, desc, _ = _data(nxy, nt)
    desc = desc[:70]
    pick = np.array([9, 40, 9, 0, 69, 40, 17, 3, 3, 33] + list(range(70)))   # copies before and after the first one
    words, dist = _assign(gpu, desc, desc[pick], nxy, nt)
    assert (dist == 0).all()
    segs = tracking._channel_slices(_layout(nxy, nt))
    for i in range(70):   # the first copy: no earlier word equals the descriptor in that channel
        for c, seg in enumerate(segs):
            same = (desc[pick][:, seg] == desc[i, seg]).all(1)
            assert words[i, c] == np.flatnonzero(same)[0], (i, c)


@pytest.mark.parametrize("size", LAYOUTS + STRUCTURED_LAYOUTS, ids=_id)
def test_an_asymmetric_codebook_and_the_corners_of_the_signed_domain(gpu, size):
    """word k differs from the base row only in entry k mod n_c of every channel; descriptor i differs from it in entry
    (3 i + 1) mod n_c by twice as much: its nearest words are exactly those with k = 3 i + 1 (mod n_c), at distance 1 -- a
    kernel that swaps words and tracks, rows and columns or k-steps does not find them.  Then 0 and 255 against 255 and 0."""
    nxy, nt = size
    layout = _layout(nxy, nt)
    segs = tracking._channel_slices(layout)
    rng = np.random.default_rng(5)
    base = rng.integers(10, 240, layout["dims"]).astype(np.uint8)
    nwords, ntracks = 41, 35
    cb, desc = np.tile(base, (nwords, 1)), np.tile(base, (ntracks, 1))
    for seg in segs:
        n_c = seg.stop - seg.start
        for k in range(nwords):
            cb[k, seg.start + k % n_c] += 1
        for i in range(ntracks):
            desc[i, seg.start + (3 * i + 1) % n_c] += 2
    words, dist = _assign(gpu, desc, cb, nxy, nt)
    for c, seg in enumerate(segs):
        n_c = seg.stop - seg.start
        for i in range(ntracks):
            first = [k for k in range(nwords) if k % n_c == (3 * i + 1) % n_c]
            assert (words[i, c], dist[i, c]) == ((first[0], 1) if first else (0, 5)), (i, c, words[i, c], dist[i, c])
    # the +-128 corner: all 0, all 255, and both halves
    D = layout["dims"]
    half = np.where(np.arange(D) % 2 == 0, 0, 255).astype(np.uint8)
    corner = np.stack([np.zeros(D, np.uint8), np.full(D, 255, np.uint8), half, 255 - half])
    words, dist = _assign(gpu, corner, corner[[1, 0, 3]], nxy, nt)
    assert words[:2].tolist() == [[1] * 4, [0] * 4] and (dist[:2] == 0).all()
    words, dist = _assign(gpu, corner[:1], corner[1:2], nxy, nt)
    assert dist.tolist() == [[(s.stop - s.start) * 255 * 255 for s in segs]]


# ------------------------------------------------------------------ 3. end to end behind ofdis_track_descriptors
END_TO_END_16_CELLS = (64, 48, 2, 1, 6, 3, 64, 4, 1)   # of tests/test_gpu_descriptors.py: C = 16, bof_assign_kernel<6, 3, true>
assert END_TO_END_16_CELLS in DESC_CASES


def _end_to_end(gpu, case, every):
    """descriptors of the device -> ofdis_track_bof; the codebook: every `every`-th descriptor, noise, the descriptors behind them"""
    w, h, _, _, npairs, _, N, nxy, nt = case
    frames, fw, (tracks, start, length, info), want, _ = _desc_case(*case, 1)
    n, lmax = len(length), tracks.shape[0] - 1
    layout = tracking.descriptor_layout(N, nxy, nt)
    D = layout["dims"]
    desc = tracking.normalize_descriptors_u8(want[0], layout)   # the model's own hist
    rng = np.random.default_rng(97)
    codebook = np.concatenate([desc[::every], rng.integers(0, 256, (7, D)).astype(np.uint8), desc[1::every]])
    words, _ = tracking.codebook_assign_ref(desc, layout, codebook)
    assert n >= 2 and (length >= 2).any() and want[0].any(), np.bincount(length)   # (a track of one point has a zero hist)
    dfr, dfw, dt, ds, dl, di = (gpu.Dev(a) for a in (frames, fw, tracks, start, length, info))
    dh, dc = gpu.Dev(nbytes=n * D * 4), gpu.Dev(codebook)
    for min_len in (1, 2, lmax + 1):
        db, dw = gpu.Dev(np.full(16 * len(codebook), 0xAB, np.uint8)), gpu.Dev(nbytes=n * 16)
        gpu.track_descriptors_dev(dfr.ptr, dfw.ptr, npairs, w, h, 1, dt.ptr, ds.ptr, dl.ptr, di.ptr, lmax, n, N, nxy, nt, MIN_FLOW, dh.ptr)
        gpu.track_bof_dev(dh.ptr, dl.ptr, di.ptr, n, nxy, nt, dc.ptr, len(codebook), min_len, db.ptr, dw.ptr)
        gpu.check(gpu.lib().ofdis_sync(None))
        assert np.array_equal(dw.get((n, 4), np.int32), words)
        assert np.array_equal(db.get((4, len(codebook)), np.uint32), tracking.bof_ref(words, length, len(codebook), min_len))
    return len(codebook)


def test_end_to_end_behind_the_descriptors(gpu):
    _end_to_end(gpu, min(DESC_CASES, key=lambda c: c[0] * c[1]), 3)   # the smallest gray case of tests/test_gpu_descriptors.py


def test_end_to_end_behind_the_descriptors_of_16_cells(gpu):
    """N 64, nxy 4, nt 1: the device's own hist through bof_assign_kernel<6, 3, true>, more than two of its tiles of 48 words"""
    assert _end_to_end(gpu, END_TO_END_16_CELLS, 33) > 2 * 48


# ------------------------------------------------------------------ 4. determinism and purity
def test_twice_the_same_bytes_on_a_stream_of_its_own(gpu):
    """ofdis_track_bof twice into buffers pre-filled with different garbage, on a non-default stream: the same bytes, and the
    model's"""
    nxy, nt, ntracks, nwords, min_len = 2, 3, 200, 300, 2
    _, _, length, desc, _ = _data(nxy, nt)
    words, dist, _ = _assigned(nxy, nt, nwords)
    stream = gpu.Stream()
    try:
        run = _Run(gpu, nxy, nt, ntracks, nwords, min_len, stream=stream)
        _check(run, desc, words, dist, length, min_len, "stream")
        first = {k: run.raw[k].copy() for k in ("fbof", "fwords")}
        for k in first:   # other garbage, then the same call again
            gpu.check(gpu.lib().ofdis_memcpy_h2d(run.dev[k].ptr, np.full(run.sizes[k] + GUARD, 0x5C, np.uint8).ctypes.data,
                                                 run.sizes[k] + GUARD))
        run.fused(min_len, "fbof", "fwords")
        gpu.check(gpu.lib().ofdis_sync(stream.ptr))
        for k, v in run.sizes.items():
            if k in first:
                again = run.dev[k].get((v + GUARD,), np.uint8)
                assert (again[v:] == 0x5C).all()
                body, want = again[:v], first[k][:v]
                if k == "fwords":   # the idle slots keep whatever garbage they held
                    body, want = body[:ntracks * 16], want[:ntracks * 16]
                    assert (again[ntracks * 16:v] == 0x5C).all()
                assert np.array_equal(body, want), k
    finally:
        stream.close()


def test_a_words_array_of_the_caller_with_entries_outside_the_codebook(gpu):
    """ofdis_bof_histogram on words the caller filled: entries outside 0 .. nwords-1 are not counted and nothing is written
    outside bof"""
    rng = np.random.default_rng(8)
    words = rng.integers(-3, 12, (300, 4)).astype(np.int32)
    length = rng.integers(1, 5, 300).astype(np.int32)
    for min_len in (1, 3):
        assert np.array_equal(gpu.bof_histogram(words, length, 9, min_len), tracking.bof_ref(words, length, 9, min_len))
