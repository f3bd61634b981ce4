"""The launch hooks of the TEST library (tests/csrc/ofdis_launch_hooks*.hip): the product's own launchers behind thin C wrappers, and
the two launch limits of of_dis_amd/csrc/ofdis_kernels.h -- QUAD_MAX_BLOCKS (workgroups of one launch of a quad kernel: the
launcher walks the frames in chunks) and GRID_MAX_BLOCKS (grid of a grid-stride kernel: the kernel loops) -- as variables of
that library which a test lowers.  Shared by tests/test_launch_geometry.py (CPU) and tests/test_gpu_launch_limits.py; the
pyramid's launchers and their kernel selection (pyr_base_variant, pyr_planes_variant) also by tests/pyr_classes.py,
tests/test_pyr_ref.py (CPU) and tests/test_gpu_pyramid.py; the level launchers with a free UpGeom by
tests/test_gpu_level_routes.py; the core launchers' host-only decisions (xcd_grid, slot_rows, choose_patch_kernel) by
tests/test_launch_geometry.py and tests/test_patch_kernel_choice.py.

libofdis_hip.so is a separate object with the limits compiled in as constants: nothing here changes what it does."""
import contextlib
import ctypes as C

import numpy as np

QUAD_MAX_BLOCKS, GRID_MAX_BLOCKS = 1 << 22, 1 << 20   # the product's values
_I = C.c_int


def hooks():
    """libofdis_testhooks.so, every hook with the prototype tests/csrc/ofdis_test_hooks.h declares (common.testhooks)"""
    from common import testhooks
    return testhooks()


def launch(name, *args):
    """ofdis_test_launch_<name>(*args) on the null stream; a hipError_t other than hipSuccess is a failure"""
    rc = getattr(hooks(), "ofdis_test_launch_" + name)(*args, None)
    assert rc == 0, f"ofdis_test_launch_{name}: hipError_t {rc}"


@contextlib.contextmanager
def launch_limits(quad_max_blocks=0, grid_max_blocks=0):
    """the test library's limits lowered (0: the product's value), and back at the product's values afterwards whatever happens"""
    L = hooks()
    L.ofdis_test_set_launch_limits(quad_max_blocks, grid_max_blocks)
    try:
        yield
    finally:
        L.ofdis_test_set_launch_limits(0, 0)


def quad_grid(nframes, w, h):
    """(bpf, chunk) of quad_grid(nframes, w, h) under the limits in force"""
    bpf, chunk = _I(), _I()
    hooks().ofdis_test_quad_grid(nframes, w, h, C.byref(bpf), C.byref(chunk))
    return bpf.value, chunk.value


def quad_blocks(frames, bpf):
    return int(hooks().ofdis_test_quad_blocks(frames, bpf))


def grid_for(total):
    return int(hooks().ofdis_test_grid_for(total))


def xcd_frame_map(nblocks, bpf, nframes):
    """(frame, blk) of workgroups 0 .. nblocks-1 of a launch over nframes frames, as xcd_frame_map gives them to the kernels"""
    frame, blk = np.empty(nblocks, np.int32), np.empty(nblocks, np.int32)
    hooks().ofdis_test_xcd_frame_map(0, nblocks, bpf, nframes, frame.ctypes.data, blk.ctypes.data)
    return frame, blk


def xcd_grid(nframes, blocks_per_frame):
    """workgroups of the grid xcd_grid (ofdis_dev.h) gives the core launchers whose kernels call xcd_frame_map; None: refused"""
    n = int(hooks().ofdis_test_xcd_grid(nframes, blocks_per_frame))
    return None if n < 0 else n


def slot_rows(h):
    """slot_rows (ofdis_kernels.h): rows per frame slot of a wavefront at level height h"""
    return int(hooks().ofdis_test_slot_rows(h))


PATCH_FAMILIES = ("none", "lanes16", "gray8", "generic")   # PatchKernel::Family


def patch_kernel_choice(P, noc, nop, stereo, costfct, pixw_asked, gray8, rgb12, rgb12_lpp, contract):
    """choose_patch_kernel (ofdis_kernels.h) as a dict: family (PATCH_FAMILIES), targs (the kernel's template arguments in its
    parameter order, trailing zeros cut to the family's count), lpp, threads, blocks_per_frame, pixw"""
    out = (_I * 9)()
    hooks().ofdis_test_patch_kernel_choice(P, noc, nop, int(stereo), costfct, int(pixw_asked), gray8, rgb12, rgb12_lpp, contract, out)
    family = PATCH_FAMILIES[out[0]]
    return dict(family=family, targs=tuple(out[1:5])[:{"none": 0, "gray8": 2}.get(family, 4)], lpp=out[5], threads=out[6],
                blocks_per_frame=out[7], pixw=bool(out[8]))


def chunk_walk(nframes, w, h):
    """the launches of one call, recorded from the launchers' own loop (quad_chunks, ofdis_quad.h): bpf and [(f0, n, workgroups)]"""
    bpf, _ = quad_grid(nframes, w, h)
    walk = np.empty((nframes, 3), np.int32)   # (a chunk has at least one frame)
    count = hooks().ofdis_test_quad_chunks(nframes, w, h, nframes, walk.ctypes.data)
    assert 0 <= count <= nframes, f"ofdis_test_quad_chunks: {count}"
    return bpf, [tuple(int(v) for v in row) for row in walk[:count]]


def _three(fn, C_):
    a, b, c = _I(), _I(), _I()
    fn(C_, C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def bof_shape(cells):
    """(nk, NK, TG) of bof_assign_shape(C) (ofdis_bof.hip), C = nxy^2 nt: the k-steps of the longest channel and the
    bof_assign_kernel<NK, TG, .> the launcher picks; a workgroup owns 64 TG slots and stages tiles of 16 TG words"""
    return _three(hooks().ofdis_test_bof_shape, cells)


def km_geom(cells):
    """(np, el, rl) of km_geom(C) (ofdis_kmeans.hip): the passes and lanes of the update's sum, the entries of a slab row"""
    return _three(hooks().ofdis_test_km_geom, cells)


def km_finish_split(n_c):
    """the entries km_finish_kernel's 256 threads take at a time on a channel of n_c entries: 16, 128 or 256"""
    return int(hooks().ofdis_test_km_finish_split(n_c))


def pyr_base_variant(address, wo, W, noc, l, pitch, stride):
    """pyr_base_variant (ofdis_pyr.hip) for frames at `address` (only its alignment matters): 0 = pyr_base_kernel, 4 / 8 / 16 =
    pyr_base16_kernel of that block size"""
    return int(hooks().ofdis_test_pyr_base_variant(address, wo, W, noc, l, pitch, stride))


def pyr_planes_variant(w, h, noc, pad, want_down):
    """pyr_planes_variant (ofdis_pyr.hip): 0 = pyr_planes_kernel (and a pyr_down launch where `down` is wanted), 1 =
    pyr_planes_gray4_kernel, 2 = pyr_planes_gray4_kernel writing `down` too"""
    return int(hooks().ofdis_test_pyr_planes_variant(w, h, noc, pad, int(bool(want_down))))


def upsample_lr_fuses(wo):
    """upsample_lr_fuses (ofdis_stereo_lr.hip): whether ofdis_batch_upsample_lr takes the fused kernel at original width wo"""
    return bool(hooks().ofdis_test_upsample_lr_fuses(wo))


def trips(total):
    """grid-stride trips of the busiest thread over `total` elements under the limits in force"""
    return -(-total // (256 * grid_for(total)))
