"""-m gpu: the five kernels of the image pyramid (of_dis_amd/csrc/ofdis_pyr.hip), each launcher through its hook of the test library,
against the exact reference tests/pyr_ref.py -- byte equality on every output, no tolerance.

The cases are the lists of tests/pyr_classes.py, which tests/test_pyr_ref.py holds to a member of every selection class (which
kernel a launcher picks; how many blocks of pyr_base_kernel take its word path).  That a case runs the kernel it is named for
is asserted on the launchers' own variant functions, never on the kernel under test.

Buffers.  Every output is pre-filled with 0xAB and lies between two guards of 0xAB.  Every input is seeded random bytes,
between the rows and between the frames too, and lies between random bytes: a read outside a row changes a sum.  An output the
call must not write (`down` not asked for, gradients not asked for) is passed as a null pointer, so a kernel that wrote it
anyway would have to hit a neighbour's guard.  The expected bytes come from pyr_ref, never from another GPU run."""
import numpy as np
import pytest

import oracle
import pyr_classes as PC
import pyr_ref
from launch_hooks import hooks, launch, pyr_base_variant, pyr_planes_variant
from of_dis_amd.params import oppoint, padded_size

pytestmark = pytest.mark.gpu
_f32 = np.float32
AB, GUARD = 0xAB, 512
HIP_ERROR_INVALID_VALUE = 1


class Out:
    """a float32 device array pre-filled with 0xAB between two guards of 0xAB"""

    def __init__(self, gpu, shape):
        self.shape = tuple(shape)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * 4
        self.dev = gpu.Dev(np.full(self.nbytes + 2 * GUARD, AB, np.uint8))
        self.ptr = self.dev.ptr + GUARD

    def get(self, what):
        raw = self.dev.get((self.nbytes + 2 * GUARD,), np.uint8)
        assert (raw[:GUARD] == AB).all(), f"{what}: written before the start of the array"
        assert (raw[GUARD + self.nbytes:] == AB).all(), f"{what}: written past the end of the array"
        return raw[GUARD:GUARD + self.nbytes].view(_f32).reshape(self.shape)


class In:
    """a device copy of `arr` between two stretches of random bytes (finite as floats: every byte below 0x7f)"""

    def __init__(self, gpu, arr, rng):
        arr = np.ascontiguousarray(arr)
        raw = np.concatenate([rng.integers(0, 0x7f, GUARD, dtype=np.uint8), arr.view(np.uint8).ravel(),
                              rng.integers(0, 0x7f, GUARD, dtype=np.uint8)])
        self.dev = gpu.Dev(raw)
        self.ptr = self.dev.ptr + GUARD


def assert_same_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == _f32, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = (np.ascontiguousarray(a).view(np.uint32) for a in (got, want))
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        unwritten = int((g[g != w] == 0xABABABAB).sum())
        raise AssertionError(f"{what}: {len(bad)} of {g.size} values differ ({unwritten} of them never written), in frames "
                             f"{sorted(set(bad[:, 0].tolist()))}; first at {i}: {got[i]!r} ({g[i]:#010x}) vs {want[i]!r} ({w[i]:#010x})")


def sync(gpu):
    gpu.check(gpu.lib().ofdis_sync(None))


def _seed(case):
    return sum((k + 1) * (v if isinstance(v, int) else len(str(v))) for k, v in enumerate(case)) + 99


# ------------------------------------------------------------------ launch_pyr_base
def _base_buffer(c, rng):
    """the bytes of a case: random everywhere (frames, gaps between rows and frames, the `offset` bytes in front), then the
    rows of a frame overwritten for the contents that are not random"""
    pitch, stride, span = PC.base_layout(c)
    buf = rng.integers(0, 256, c.offset + span, dtype=np.uint8)
    if c.content != "random":
        bs = 1 << c.l
        left, top = (c.W - c.wo) // 2, (c.H - c.ho) // 2
        yy, xx = np.mgrid[0:c.ho, 0:c.wo]
        checker = ((((yy + top) // bs) + ((xx + left) // bs)) & 1) * 255   # blocks of the padded frame are all 0 or all 255
        for f in range(c.nframes):
            frame = {"all255": np.full((c.ho, c.wo), 255), "all0": np.zeros((c.ho, c.wo), int),
                     "checker": checker if f != 1 else 255 - checker}[c.content].astype(np.uint8)
            for y in range(c.ho):
                o = c.offset + f * stride + y * pitch
                buf[o:o + c.wo] = frame[y]
    return buf


@pytest.mark.parametrize("c", PC.BASE_CASES, ids=lambda c: c.name)
def test_pyr_base(gpu, c):
    rng = np.random.default_rng(_seed(c[1:10]))
    pitch, stride, _ = PC.base_layout(c)
    buf = _base_buffer(c, rng)
    want = pyr_ref.base(buf, c.nframes, c.wo, c.ho, c.W, c.H, c.noc, c.l, pitch, stride, c.offset)
    if c.content == "checker":
        assert set(np.unique(want).tolist()) == {0.0, 255.0}
    src = In(gpu, buf, rng)
    assert src.ptr % 16 == 0
    # the kernel this case is named for, at the address the launcher really gets
    variant = pyr_base_variant(src.ptr + c.offset, c.wo, c.W, c.noc, c.l, pitch, stride)
    assert (variant, c.noc) == PC.base_class(c)[:2]
    if c.name.startswith("stream"):
        assert variant == 1 << c.l
    if "demoted" in c.name:
        assert variant == 0 and pyr_base_variant(src.ptr, c.wo, c.W, c.noc, c.l, pitch, stride) == 4
    out = Out(gpu, want.shape)
    launch("pyr_base", src.ptr + c.offset, out.ptr, c.nframes, c.wo, c.ho, c.W, c.H, c.noc, c.l, pitch, stride)
    sync(gpu)
    assert_same_bytes(out.get(c.name), want, c.name)


# ------------------------------------------------------------------ launch_pyr_down, launch_pyr_planes
def _level_images(rng, n, w, h, noc, content):
    """unpadded level images [n][h][w][noc]: "u8" = what level 7 of 8-bit frames can hold (multiples of 4^-7 up to 255: the
    hardest values of the exactness claim), "float" = arbitrary float32 of both signs and many magnitudes"""
    if content == "u8":
        v = rng.integers(0, 255 * 4 ** 7 + 1, (n, h, w, noc)).astype(np.float64) / 4.0 ** 7
        v.flat[::5] = np.round(v.flat[::5])   # and plain integers between them, 0 and 255 among them
        v.flat[::17] = 255.0
        v.flat[3::17] = 0.0
        return pyr_ref.f32_exact(v, "level-7 values")
    return (rng.standard_normal((n, h, w, noc)) * 10.0 ** rng.integers(-3, 4, (n, h, w, noc))).astype(_f32)


@pytest.mark.parametrize("c", PC.DOWN_CASES, ids=lambda c: f"{c.w}x{c.h}x{c.noc}-{c.content}")
def test_pyr_down(gpu, c):
    rng = np.random.default_rng(_seed(c))
    src = _level_images(rng, PC.NFRAMES, c.w, c.h, c.noc, c.content)
    want = pyr_ref.down(src)
    assert want.shape == (PC.NFRAMES, c.h // 2, c.w // 2, c.noc) and want.size
    dev, out = In(gpu, src, rng), Out(gpu, want.shape)
    launch("pyr_down", dev.ptr, out.ptr, PC.NFRAMES, c.w, c.h, c.noc)
    sync(gpu)
    assert_same_bytes(out.get("down"), want, "down")


def _planes_id(c):
    return f"{c.w}x{c.h}x{c.noc}-pad{c.pad}-{'grad' if c.grad else 'nograd'}-{'down' if c.down else 'nodown'}-{c.content}"


@pytest.mark.parametrize("c", PC.PLANES_CASES, ids=_planes_id)
def test_pyr_planes(gpu, c):
    rng = np.random.default_rng(_seed(c))
    n = PC.NFRAMES
    src = _level_images(rng, n, c.w, c.h, c.noc, c.content)
    want = dict(zip(("image", "dx", "dy"), pyr_ref.planes(src, c.pad, c.grad)))
    if c.down:
        want["down"] = pyr_ref.down(src)
    assert pyr_planes_variant(c.w, c.h, c.noc, c.pad, c.down) == PC.planes_class(c)[0]
    dev = In(gpu, src, rng)
    # allocated in this order whether they are passed or not: an output that is not asked for is a null pointer, and the
    # arrays that are keep their guards
    outs = {name: Out(gpu, (n, c.h + 2 * c.pad, c.w + 2 * c.pad, c.noc)) for name in ("image", "dx", "dy")}
    outs["down"] = Out(gpu, (n, max(c.h // 2, 1), max(c.w // 2, 1), c.noc))
    ptr = lambda name: outs[name].ptr if want.get(name) is not None else None
    launch("pyr_planes", dev.ptr, ptr("image"), ptr("dx"), ptr("dy"), ptr("down"), n, c.w, c.h, c.noc, c.pad)
    sync(gpu)
    for name, out in outs.items():
        got = out.get(name)
        if want.get(name) is None:
            assert (got.view(np.uint32) == 0xABABABAB).all(), f"{name}: written although it was not asked for"
        else:
            assert_same_bytes(got, want[name], name)


def test_pyr_planes_rejects_what_its_grid_cannot_carry():
    """host only: the launcher returns before anything is launched (the frames ride in grid.y, a frame's elements in 32 bits)"""
    L = hooks()
    assert L.ofdis_test_launch_pyr_planes(None, None, None, None, None, 65536, 8, 2, 1, 4, None) == HIP_ERROR_INVALID_VALUE
    side = 46341   # 46341^2 = 2^31 + 4633
    assert side * side >= 1 << 31 > (side - 1) * (side - 1)
    for w, h, noc, pad in ((side, side, 1, 0), (side - 8, side - 8, 1, 4), (1 << 16, 1 << 15, 1, 0), (26755, 26755, 3, 0)):
        assert (w + 2 * pad) * (h + 2 * pad) * noc >= 1 << 31
        assert L.ofdis_test_launch_pyr_planes(None, None, None, None, None, 1, w, h, noc, pad, None) == HIP_ERROR_INVALID_VALUE, (w, h)


# ------------------------------------------------------------------ the whole call
KINDS = ("image A", "dx A", "dy A", "image B", "dx B", "dy B")


def _read_planes(gpu, b, p, level, kind, nframes):
    ptr = b.input_ptr(level, kind)
    assert ptr, (level, kind)
    a = np.empty((nframes,) + p.plane_shape(level), _f32)
    assert a[0].size == b.input_elems(level)
    gpu.check(gpu.lib().ofdis_memcpy_d2h(a.ctypes.data, ptr, a.nbytes))
    return a


def _params(opp, w, h, noc, fb=0):
    p = oppoint(opp, w, h, noc=noc).copy(usefbcon=fb)
    p.width, p.height = padded_size(w, h, p.sc_f)
    return p


def _frames(rng, n, w, h, noc):
    return rng.integers(0, 256, (n, h, w) + ((3,) if noc == 3 else ()), dtype=np.uint8)


def _expected(p, frames):
    """per frame {level: planes} from pyr_ref, with the oracle asserted beside it"""
    levels = range(p.sc_l, p.sc_f + 1)
    want = [pyr_ref.pyramid(f, p.width, p.height, levels, p.imgpadding) for f in frames]
    O = oracle.c_oracle()
    for f, w in zip(frames, want):
        orc = O.build_pyramid(p, f)
        for l in levels:
            for k in range(3):
                assert np.array_equal(orc[k][l].view(np.uint32), w[l][k].view(np.uint32)), (l, k)
    return want


@pytest.mark.parametrize("noc,opp,w,h,fb", [(3, 3, 90, 70, 0), (1, 2, 250, 109, 0), (1, 2, 250, 109, 1)],
                         ids=["rgb-90x70-op3", "gray-250x109-op2", "gray-250x109-op2-fb"])
def test_build_pyramids_u8(gpu, noc, opp, w, h, fb):
    """every plane kind of every level of a pair context: A with gradients, B without them unless usefbcon asks for them"""
    rng = np.random.default_rng(w * h + fb)
    p = _params(opp, w, h, noc, fb)
    n = 3
    fa, fbk = _frames(rng, n, w, h, noc), _frames(rng, n, w, h, noc)
    wa, wb = _expected(p, fa), _expected(p, fbk)
    b = gpu.Batch(p, n)
    da, db = gpu.Dev(fa), gpu.Dev(fbk)
    b.build_pyramids_u8(da.ptr, db.ptr, w, h)
    sync(gpu)
    for l in range(p.sc_l, p.sc_f + 1):
        for kind in range(6):
            if kind >= 4 and not fb:
                assert not b.input_ptr(l, kind)
                continue
            want = np.stack([(wa if kind < 3 else wb)[f][l][kind % 3] for f in range(n)])
            assert_same_bytes(_read_planes(gpu, b, p, l, kind, n), want, f"level {l} {KINDS[kind]}")
    b.close()


def test_build_pyramids_u8_seq(gpu):
    """a sequence context of two pairs: three frame slots, each frame through the pyramid once, with its gradients; the B side
    of pair k is frame slot k + 1.  320 wide: the streaming base kernel and the quad kernel with fused down"""
    w, h, n = 320, 50, 2
    rng = np.random.default_rng(320)
    p = _params(2, w, h, 1)
    assert (p.sc_l, p.sc_f, p.width, p.height) == (2, 4, 320, 64)
    frames = _frames(rng, n + 1, w, h, 1)
    want = _expected(p, frames)
    b = gpu.Batch(p, n, sequence=True)
    assert b.input_frames() == n + 1
    d = gpu.Dev(frames)
    b.build_pyramids_u8_seq(d.ptr, w, h)
    sync(gpu)
    for l in range(p.sc_l, p.sc_f + 1):
        for kind in range(3):
            got = _read_planes(gpu, b, p, l, kind, n + 1)
            assert_same_bytes(got, np.stack([want[f][l][kind] for f in range(n + 1)]), f"level {l} {KINDS[kind]}, slots 0..{n}")
            assert b.input_ptr(l, 3 + kind) == b.input_ptr(l, kind) + 4 * b.input_elems(l)   # B of pair k = slot k + 1
    b.close()
