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
import functools

import numpy as np

QUAD_MAX_BLOCKS, GRID_MAX_BLOCKS = 1 << 22, 1 << 20   # the product's values
_I, _F, _VP, _LL, _SZ = C.c_int, C.c_float, C.c_void_p, C.c_longlong, C.c_size_t
_UPG = [_I] * 7   # UpGeom: sw, sh, sc_l, left, top, wo, ho

_SIGNATURES = {
    "interp_frames": [_VP] * 7 + [_I] * 4 + [_VP, _I, _VP],
    "interp_bidir": [_VP] * 5 + [_I] + _UPG + [_I, _VP, _I, _F, _F, _VP],
    "tfilter_frames": [_VP] * 7 + [_I] * 4 + [_F, _F, _VP],
    "tfilter_level": [_VP] * 5 + [_I] + _UPG + [_I, _F, _F, _F, _F, _VP],
    "trajfilter_frames": [_VP] * 5 + [_I] * 4 + [_VP, _I, _F, _I, _F, _F, _VP],
    "trajfilter_level": [_VP] * 5 + [_I] + _UPG + [_I, _VP, _I, _F, _I, _F, _F, _VP],
    "gmotion_frames": [_VP, _VP] + [_I] * 5 + [_F, _VP, _VP, _VP, _VP],
    "gmotion_compensate_frames": [_VP] * 3 + [_I] * 3 + [_F, _VP, _VP, _VP],
    "gmotion_level": [_VP, _VP, _I] + _UPG + [_I, _I, _F, _F, _F, _VP, _VP, _VP, _VP],
    "gmotion_compensate_level": [_VP] * 3 + [_I] + _UPG + [_F, _F, _F, _VP, _VP, _VP],
    "warp_frames": [_VP] * 4 + [_I] * 5 + [_VP],
    "pyr_base": [_VP, _VP] + [_I] * 7 + [_SZ, _SZ, _VP],
    "pyr_down": [_VP, _VP] + [_I] * 4 + [_VP],
    "pyr_planes": [_VP] * 5 + [_I] * 5 + [_VP],
    "encode": [_VP, _VP, _SZ, _I, _F, _F, _VP],
    "fb_check": [_VP] * 3 + [_I] * 3 + [_F, _F, _VP],
    "mirror_u8": [_VP, _VP] + [_I] * 4 + [_VP],
    "lr_check": [_VP] * 3 + [_I] * 3 + [_F, _F, _VP],
    "disparity_fill": [_VP] * 3 + [_I] * 4 + [_VP],
    # tests/csrc/ofdis_launch_hooks_levels.hip
    "upsample_crop_enc": [_VP, _VP, _I] + _UPG + [_I, _I, _F, _F, _VP],
    "upsample_bidir": [_VP] * 6 + [_I] + _UPG + [_F, _F, _VP],
    "projective_level": [_VP, _VP, _I] + _UPG + [_I, _F, _F, _F, _VP, _VP, _VP, _VP],
    "projective_compensate_level": [_VP] * 3 + [_I] + _UPG + [_F, _F, _F, _VP, _VP, _VP],
    "track_level": [_VP, _VP, _I] + _UPG + [_VP, _VP, _I, _I, _F, _F, _VP, _VP, _VP],
    "dense_tracks_level": [_VP] * 3 + [_I] + _UPG + [_I] * 5 + [_F, _F, _I] + [_VP] * 6,
    "upsample_lr": [_VP] * 6 + [_I] + _UPG + [_I, _F, _F, _VP],
    "lr_materialise": [_VP] * 4 + [_I] + _UPG + [_VP],
}


@functools.lru_cache(maxsize=None)
def hooks():
    """libofdis_testhooks.so with the launch hooks' signatures.  No fallback: a library without them is a failure."""
    from common import testhooks
    L = testhooks()
    for name, argtypes in _SIGNATURES.items():
        fn = getattr(L, "ofdis_test_launch_" + name)
        fn.argtypes, fn.restype = argtypes, _I
    L.ofdis_test_set_launch_limits.argtypes, L.ofdis_test_set_launch_limits.restype = [_LL, _LL], None
    L.ofdis_test_quad_grid.argtypes, L.ofdis_test_quad_grid.restype = [_I, _I, _I, C.POINTER(_I), C.POINTER(_I)], None
    L.ofdis_test_quad_blocks.argtypes, L.ofdis_test_quad_blocks.restype = [_I, _I], C.c_uint
    L.ofdis_test_quad_chunks.argtypes, L.ofdis_test_quad_chunks.restype = [_I, _I, _I, _I, _VP], _I
    L.ofdis_test_grid_for.argtypes, L.ofdis_test_grid_for.restype = [_LL], C.c_uint
    L.ofdis_test_xcd_frame_map.argtypes, L.ofdis_test_xcd_frame_map.restype = [_I, _I, _I, _I, _VP, _VP], None
    L.ofdis_test_xcd_grid.argtypes, L.ofdis_test_xcd_grid.restype = [_I, _LL], _LL
    L.ofdis_test_slot_rows.argtypes, L.ofdis_test_slot_rows.restype = [_I], _I
    L.ofdis_test_patch_kernel_choice.argtypes, L.ofdis_test_patch_kernel_choice.restype = [_I] * 10 + [C.POINTER(_I)], None
    L.ofdis_test_gmotion_work_bytes.argtypes, L.ofdis_test_gmotion_work_bytes.restype = [_I, _I, _I], _SZ
    L.ofdis_test_bof_shape.argtypes, L.ofdis_test_bof_shape.restype = [_I] + [C.POINTER(_I)] * 3, None
    L.ofdis_test_km_geom.argtypes, L.ofdis_test_km_geom.restype = [_I] + [C.POINTER(_I)] * 3, None
    L.ofdis_test_km_finish_split.argtypes, L.ofdis_test_km_finish_split.restype = [_I], _I
    L.ofdis_test_pyr_base_variant.argtypes, L.ofdis_test_pyr_base_variant.restype = [_VP] + [_I] * 4 + [_SZ, _SZ], _I
    L.ofdis_test_pyr_planes_variant.argtypes, L.ofdis_test_pyr_planes_variant.restype = [_I] * 5, _I
    L.ofdis_test_upsample_lr_fuses.argtypes, L.ofdis_test_upsample_lr_fuses.restype = [_I], _I
    return L


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
