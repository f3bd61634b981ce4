"""CPU: the exact pyramid reference (tests/pyr_ref.py) against the C restatement (oracle/ofdis_oracle.c), bit for bit, and the
case lists of tests/test_gpu_pyramid.py against the selection classes of the pyramid's launchers (tests/pyr_classes.py).

Two restatements of the same documented arithmetic -- OpenCV's resize(0.5, INTER_LINEAR), Sobel(ksize 3, scale 1/8,
BORDER_DEFAULT) and copyMakeBorder -- written independently: the oracle follows the library's operation order in float32, the
reference here computes integer block sums in int64 and the Sobel in float64 and asserts that every value is representable in
float32.  They agree on every bit, signed zeros included, or one of them is wrong.  No tolerance anywhere.

The class coverage: a class is what a launcher, or a kernel per block, does differently from one geometry to the next.  The
classes come from the launchers' own functions through the test library's host-only hooks; removing a case from a list so
that a class loses its last member fails here."""
import os

import numpy as np
import pytest

import oracle
import pyr_classes as PC
import pyr_ref
from of_dis_amd.params import oppoint, padded_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} values differ in their bits; first at {i}: {got[i]!r} vs {want[i]!r}")


def _content(kind, rng, w, h, noc, block):
    shape = (h, w) + ((3,) if noc == 3 else ())
    if kind == "all0":
        return np.zeros(shape, np.uint8)
    if kind == "all255":
        return np.full(shape, 255, np.uint8)
    if kind == "checker":   # 0 / 255 squares of the coarsest level's block: the largest differences between neighbours
        yy, xx = np.mgrid[0:h, 0:w]
        img = ((((yy // block) + (xx // block)) & 1) * 255).astype(np.uint8)
        return img if noc == 1 else np.stack([img, 255 - img, img], axis=-1)
    return rng.integers(0, 256, shape, dtype=np.uint8)


def _sweep():
    """40 seeded cases: gray and RGB, operating points 1 to 4, odd and even sizes from 40 to 400 pixels, frames lower than a
    block of the coarsest level, and all-0, all-255 and block-checkerboard content between the random ones"""
    rng = np.random.default_rng(20240)
    cases = []
    for k in range(40):
        noc = 3 if k % 3 == 2 else 1
        opp = 1 + k % 4
        w, h = int(rng.integers(40, 401)), int(rng.integers(40, 401))
        if k % 8 == 5:
            h = int(rng.integers(1, 4))          # lower than a block of any coarsest level above 1
        if k % 2:
            w, h = w | 1, h if k % 8 == 5 else h | 1
        content = {7: "all0", 15: "all255", 23: "checker", 31: "checker"}.get(k, "random")
        cases.append(pytest.param(noc, opp, w, h, content, 3000 + k, id=f"{k}-{'rgb' if noc == 3 else 'gray'}-op{opp}-{w}x{h}-{content}"))
    return cases


def _compare_with_oracle(p, img):
    ref = pyr_ref.pyramid(img, p.width, p.height, range(p.sc_f + 1), p.imgpadding)
    orc = oracle.c_oracle().build_pyramid(p, img)
    for l in range(p.sc_f + 1):
        for kind, name in enumerate(("image", "dx", "dy")):
            assert_same_bits(ref[l][kind], orc[kind][l], f"level {l} {name}")
        pad = p.imgpadding
        assert_same_bits(ref[l][3], ref[l][0][pad:-pad, pad:-pad], f"level {l} unpadded image")


@pytest.mark.parametrize("noc,opp,w,h,content,seed", _sweep())
def test_reference_equals_the_oracle(noc, opp, w, h, content, seed):
    p = oppoint(opp, w, h, noc=noc)
    assert 0 <= p.sc_f <= 7 and (p.width, p.height) == padded_size(w, h, p.sc_f)
    img = _content(content, np.random.default_rng(seed), w, h, noc, 1 << p.sc_f)
    if h < (1 << p.sc_f):
        assert p.height == 1 << p.sc_f   # the whole frame is lower than one block of the coarsest level
    _compare_with_oracle(p, img)


@pytest.mark.parametrize("content,w,h", [("all255", 256, 256), ("checker", 256, 256), ("random", 256, 256), ("step", 512, 256),
                                         ("random", 384, 128)])
def test_reference_equals_the_oracle_at_level_7(content, w, h):
    """sc_f = 7 is the launcher's limit: the largest block sums (2^14 * 255) and, with a 0 / 255 step between blocks, the
    largest gradients.  (A level of two pixels across has no gradient at all: both neighbours are the same reflected pixel.)"""
    p = oppoint(2, w, h)
    p.sc_f, p.sc_l = 7, 5
    p.width, p.height = padded_size(w, h, 7)
    if content == "step":
        img = np.zeros((h, w), np.uint8)
        img[:, w // 2:] = 255
    else:
        img = _content(content, np.random.default_rng(77), w, h, 1, 64)   # 64: level 6 sees uniform blocks, level 7 mixed ones
    _compare_with_oracle(p, img)
    top = pyr_ref.pyramid(img, p.width, p.height, [7], 4)[7]
    if content == "step":
        assert top[3].max() == 255.0 and np.abs(top[1]).max() == 255.0 * 4 / 8 and not top[2].any()
    if w == 256:
        assert not top[1].any() and not top[2].any()


def test_level_8_is_outside_the_exactness_domain():
    """the header's limit is real: at l = 8 a Sobel sum can need more than 24 bits, and the reference says so instead of
    rounding.  0 on the left, 255 on the right with one pixel of 254: 2 * 255 + 2 * (255 - 2^-16) = 1020 - 2^-15 has 25"""
    img = np.zeros((512, 1024), np.uint8)   # (a level needs three pixels across to have a gradient)
    img[:, 512:] = 255
    img[0, 512] = 254
    with pytest.raises(AssertionError, match="not representable"):
        pyr_ref.pyramid(img, 1024, 512, [8], 4)
    pyr_ref.pyramid(img, 1024, 512, [7], 4)


@pytest.mark.parametrize("shape", [(7, 9, 1), (1, 5, 1), (4, 1, 3), (1, 1, 1), (2, 2, 3), (33, 20, 3)])
def test_sobel_equals_scipy(shape):
    """the index arithmetic of reflect-101 against scipy.ndimage's "mirror", which is the same border by another hand"""
    ndimage = pytest.importorskip("scipy.ndimage")
    v = np.random.default_rng(sum(shape)).integers(0, 256 * 16, shape).astype(np.float64) / 16
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.float64) / 8
    gx, gy = pyr_ref.sobel(v)
    for c in range(shape[2]):
        assert np.array_equal(gx[:, :, c], ndimage.correlate(v[:, :, c], kx, mode="mirror"))
        assert np.array_equal(gy[:, :, c], ndimage.correlate(v[:, :, c], kx.T, mode="mirror"))
    fx, fy = pyr_ref.sobel_f32(v.astype(np.float32))   # the kernels' float32 order: the same bits on 8-bit-derived data
    assert np.array_equal(fx, gx.astype(np.float32)) and np.array_equal(fy, gy.astype(np.float32))


def test_the_stages_compose_to_the_pyramid():
    """base, down and planes -- what the per-kernel GPU tests compare with -- give the planes of pyramid(), through a pitched
    buffer with random bytes between rows and frames"""
    rng = np.random.default_rng(5)
    n, wo, ho, W, H, noc, pad = 2, 21, 13, 24, 16, 3, 4
    pitch, stride, offset = wo * noc + 5, (wo * noc + 5) * ho + 7, 3
    buf = rng.integers(0, 256, offset + n * stride, dtype=np.uint8)
    frames = pyr_ref.frames_of(buf, n, wo, ho, noc, pitch, stride, offset)
    level = pyr_ref.base(buf, n, wo, ho, W, H, noc, 1, pitch, stride, offset)
    for l in (1, 2, 3):
        img, dx, dy = pyr_ref.planes(level, pad)
        for f in range(n):
            want = pyr_ref.pyramid(frames[f], W, H, [l], pad)[l]
            for got, w, name in zip((img[f], dx[f], dy[f], level[f]), want, ("image", "dx", "dy", "unpadded")):
                assert_same_bits(got, w, f"level {l} frame {f} {name}")
        assert pyr_ref.planes(level, pad, gradients=False)[1:] == (None, None)
        level = pyr_ref.down(level)


# ------------------------------------------------------------------ the case lists reach every class
def test_the_base_cases_have_a_member_of_every_class():
    universe = PC.base_universe()
    assert universe == {(4, 1, "-"), (8, 1, "-"), (16, 1, "-"), (0, 1, "all"), (0, 1, "some"), (0, 1, "none"), (0, 3, "none")}
    have = {PC.base_class(c) for c in PC.BASE_CASES}
    assert have == universe, (sorted(universe - have, key=repr), sorted(have - universe, key=repr))


def test_the_base_cases_are_what_their_names_say():
    by = {c.name: c for c in PC.BASE_CASES}
    for bs in (4, 8, 16):
        assert PC.base_class(by[f"stream{bs}-packed"]) == PC.base_class(by[f"stream{bs}-pitch48"]) == (bs, 1, "-")
    for o in (1, 2, 4, 8):   # one misaligned base address demotes an otherwise streamable case
        c = by[f"gray-offset{o}-demoted"]
        assert PC.base_class(c._replace(offset=0))[0] == 4 and PC.base_class(c)[0] == 0
    pitch, stride, _ = PC.base_layout(by["gray-left4-l2-blocks-in-or-out"])
    blocks = PC.word_path_blocks(PC.ALIGNED, 3, 24, 16, 32, 24, 1, 2, pitch, stride)
    assert blocks[:, 1:5, 1:7].all() and blocks.sum() == 3 * 4 * 6            # exactly the blocks inside the frame
    blocks = PC.word_path_blocks(PC.ALIGNED, 3, 24, 16, 32, 24, 1, 3, pitch, stride)
    assert blocks.sum() == 3 * 2 and blocks[:, 1, 1:3].all()                  # the others straddle the frame's edge
    c = by["gray-stride-2-mod-4"]
    pitch, stride, _ = PC.base_layout(c)
    blocks = PC.word_path_blocks(PC.ALIGNED, c.nframes, c.wo, c.ho, c.W, c.H, 1, c.l, pitch, stride)
    assert [bool(b.any()) for b in blocks] == [True, False, True, False, True]   # every other frame starts off a word
    for name in ("gray-left1-no-block-aligned", "gray-odd-pitch", "gray-l0", "gray-l1", "gray-frame-smaller-than-a-block",
                 "gray-l7-all255", "gray-l7-checker"):
        assert PC.base_class(by[name]) == (0, 1, "none"), name
    assert PC.base_class(by["gray-every-block-inside"]) == (0, 1, "all")
    assert len(by) == len(PC.BASE_CASES)


def test_the_planes_cases_have_a_member_of_every_class():
    sweep = list(PC.planes_sweep())
    classes = {PC.planes_class(c) for c in sweep}
    # generic: gray / RGB x gradients x down no / separate; quads: gradients x down no; quads with down: gradients
    assert len(classes) == 12 and {k[0] for k in classes} == {0, 1, 2}
    assert {k for k in classes if k[0]} == {(1, 1, g, "no") for g in (True, False)} | {(2, 1, g, "fused") for g in (True, False)}
    for key in (PC.planes_class, PC.why_generic, PC.vector_quads):
        assert not PC.missing(PC.PLANES_CASES, sweep, key), (key.__name__, PC.missing(PC.PLANES_CASES, sweep, key))
    assert {PC.why_generic(c) for c in sweep} - {None} == {"w % 4", "pad % 4", "w < 8", "h < 2", "odd h with down"}
    assert {PC.vector_quads(c) for c in sweep} == {None, "none", "some"}


def test_the_planes_cases_are_what_the_issue_names():
    P = PC.PlanesCase
    assert PC.planes_class(P(16, 6, 1, 4, False, True)) == (2, 1, False, "fused")      # need_lo: the lower row on even rows only
    assert PC.planes_class(P(16, 5, 1, 8, True, True)) == (0, 1, True, "separate")     # odd h: no quad kernel with down wanted
    assert PC.planes_class(P(16, 5, 1, 8, True, False)) == (1, 1, True, "no")          # ... but without it
    assert PC.vector_quads(P(8, 2, 1, 4, True, False)) == "none" and PC.vector_quads(P(12, 2, 1, 4, True, False)) == "some"
    assert PC.why_generic(P(8, 1, 1, 4, True, False)) == "h < 2" and PC.why_generic(P(4, 4, 1, 4, True, True)) == "w < 8"
    quads = (64 + 24) // 4 * (3 + 24)
    assert 512 < quads < 768 and quads % 256                                            # three workgroups, the last one ragged
    for c in (P(1, 3, 1, 2, True, False), P(3, 1, 1, 2, True, False), P(2, 2, 1, 1, True, False), P(2, 2, 3, 1, True, False)):
        assert c in PC.PLANES_CASES and PC.planes_class(c)[0] == 0
    assert any(PC.planes_class(c) == (0, 1, True, "separate") for c in PC.PLANES_CASES)
    assert len(set(PC.PLANES_CASES)) == len(PC.PLANES_CASES)


def _classes_of(cases, key):
    return sorted({key(c) for c in cases} - {None}, key=repr)


@pytest.mark.parametrize("lost", _classes_of(PC.BASE_CASES, PC.base_class), ids=repr)
def test_base_cases_without_a_class_are_noticed(lost):
    rest = [c for c in PC.BASE_CASES if PC.base_class(c) != lost]
    assert {PC.base_class(c) for c in rest} == PC.base_universe() - {lost}


@pytest.mark.parametrize("key", [PC.planes_class, PC.why_generic, PC.vector_quads], ids=lambda k: k.__name__)
def test_planes_cases_without_a_class_are_noticed(key):
    sweep = list(PC.planes_sweep())
    for lost in _classes_of(PC.PLANES_CASES, key):
        rest = [c for c in PC.PLANES_CASES if key(c) != lost]
        assert PC.missing(rest, sweep, key) == [lost], (lost, PC.missing(rest, sweep, key))


def test_the_variant_hooks_state_the_documented_rules():
    """pyr_planes_variant and pyr_base_variant over the sweeps, against the conditions the kernels' comments give"""
    for c in PC.planes_sweep():
        quads = c.noc == 1 and c.w % 4 == 0 and c.pad % 4 == 0 and c.w >= 8 and c.h >= 2
        want = (2 if quads and c.h % 2 == 0 else 0) if c.down else (1 if quads else 0)
        assert PC.planes_class(c)[0] == want, c
    for l in range(8):
        for changed, ok in (({}, True), ({"noc": 3}, False), ({"wo": 24}, False), ({"W": 72}, False), ({"pitch": 40}, False),
                            ({"stride": 168}, False), ({"offset": 8}, False), ({"pitch": 48, "stride": 256}, True)):
            c = PC.BaseCase("", 32, 5, 64, 16, 1, l)._replace(**changed)
            assert PC.base_class(c)[0] == ((1 << l) if ok and l in (2, 3, 4) else 0), (l, changed)


def test_the_table_of_the_design_document_is_the_generated_one():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert PC.table() in text, "DESIGN.md: regenerate the table with `python tests/pyr_classes.py`"
