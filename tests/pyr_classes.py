"""The selection classes of the image pyramid (of_dis_amd/csrc/ofdis_pyr.hip) and the case lists of tests/test_gpu_pyramid.py.  No GPU.

What the launchers pick is asked of the launchers' own functions through the host-only hooks of the test library
(tests/launch_hooks.py: pyr_base_variant, pyr_planes_variant).  One choice is made inside a kernel, per block: the word fast
path of pyr_base_kernel; its predicate is restated here (word_path_blocks) and a case is classed by whether all, some or none
of its blocks take it.  tests/test_pyr_ref.py holds the lists below to a member of every class; DESIGN.md (section 4, image
pyramid) has the table:

    python tests/pyr_classes.py      # prints it"""
import collections
import itertools

import numpy as np

from launch_hooks import pyr_base_variant, pyr_planes_variant

NFRAMES = 3
ALIGNED = 1 << 20   # a device address as the allocator returns it, for the host-only questions: a multiple of 16 and more

# ------------------------------------------------------------------ base level: u8 frames -> the finest level's image
# pitch = 0: packed rows (wo * noc bytes); stride = 0: packed frames (pitch * ho); offset: bytes between the (aligned) start of
# the buffer and row 0 of frame 0.  content: "random" bytes, "all255", "all0", or "checker": 0 / 255 with the period of the block
BaseCase = collections.namedtuple("BaseCase", "name wo ho W H noc l pitch stride offset content nframes",
                                  defaults=(0, 0, 0, "random", NFRAMES))
_STREAMABLE = (32, 5, 64, 16, 1)       # left 16, top 5: chunks inside the frame and in both replicated borders, rows clamped
_G = (24, 16, 32, 24, 1)               # left 4, top 4
BASE_CASES = (
    [BaseCase(f"stream{1 << l}-packed", *_STREAMABLE, l) for l in (2, 3, 4)]
    + [BaseCase(f"stream{1 << l}-pitch48", *_STREAMABLE, l, 48, 48 * 5 + 16) for l in (2, 3, 4)]
    + [BaseCase("gray-left4-l2-blocks-in-or-out", *_G, 2),
       BaseCase("gray-left4-l3-blocks-straddle", *_G, 3),
       BaseCase("gray-left1-no-block-aligned", 37, 7, 40, 8, 1, 2, 40),
       BaseCase("gray-odd-pitch", *_G, 2, 25),
       BaseCase("gray-stride-2-mod-4", *_G, 2, 24, 24 * 16 + 2, nframes=5),
       BaseCase("gray-every-block-inside", 24, 8, 24, 8, 1, 2)]
    + [BaseCase(f"gray-offset{o}-demoted", *_STREAMABLE, 2, offset=o) for o in (1, 2, 4, 8)]
    + [BaseCase(f"gray-l{l}", *_G, l) for l in (0, 1)]
    + [BaseCase(f"rgb-l{l}", 5, 3, 8, 8, 3, l) for l in (0, 1, 2, 3)]
    + [BaseCase("gray-frame-smaller-than-a-block", 3, 1, 8, 8, 1, 3),
       BaseCase("gray-l7-all255", 200, 130, 256, 256, 1, 7, content="all255"),
       BaseCase("gray-l7-checker", 200, 130, 256, 256, 1, 7, content="checker")])


def base_layout(c):
    """(pitch, stride, bytes the frames span from `offset` on) of a case"""
    pitch = c.pitch or c.wo * c.noc
    stride = c.stride or pitch * c.ho
    return pitch, stride, (c.nframes - 1) * stride + (c.ho - 1) * pitch + c.wo * c.noc


def word_path_blocks(address, nframes, wo, ho, W, H, noc, l, pitch, stride):
    """bool [nframes][H >> l][W >> l]: the blocks for which pyr_base_kernel reads whole words.  Restated from its comment: gray,
    a block of at least 4 columns entirely inside the frame, starting at a multiple of 4 columns, with the row pitch, the
    frame's offset and the base address multiples of 4 bytes"""
    bs = 1 << l
    bx0 = np.arange(W >> l) * bs - (W - wo) // 2
    by0 = np.arange(H >> l) * bs - (H - ho) // 2
    xin = (bx0 >= 0) & (bx0 + bs <= wo) & (bx0 % 4 == 0)
    yin = (by0 >= 0) & (by0 + bs <= ho)
    fin = (np.arange(nframes) * stride) % 4 == 0
    ok = noc == 1 and bs >= 4 and pitch % 4 == 0 and address % 4 == 0
    return (fin[:, None, None] & yin[None, :, None] & xin[None, None, :]) & ok


def base_class(c, address=ALIGNED):
    """(kernel, noc, word path): kernel 0 = pyr_base_kernel, 4 / 8 / 16 = pyr_base16_kernel<.>; word path "all" / "some" / "none"
    of the blocks of the generic kernel ("-" for the streaming kernel, which has none)"""
    pitch, stride, _ = base_layout(c)
    variant = pyr_base_variant(address + c.offset, c.wo, c.W, c.noc, c.l, pitch, stride)
    if variant:
        return variant, c.noc, "-"
    blocks = word_path_blocks(address + c.offset, c.nframes, c.wo, c.ho, c.W, c.H, c.noc, c.l, pitch, stride)
    return variant, c.noc, "all" if blocks.all() else "some" if blocks.any() else "none"


def base_universe():
    """every class a sweep over small geometries reaches: both channel counts, levels 0 to 4, frames that fill the working size
    or leave 1, 4 or 16 columns on the left, aligned and unaligned pitches and offsets"""
    found = set()
    for noc, l, (wo, W), (ho, H), extra, offset in itertools.product(
            (1, 3), range(5), ((32, 32), (30, 32), (24, 32), (32, 64), (48, 48)), ((16, 16), (5, 16)), (0, 1, 16), (0, 2, 4)):
        found.add(base_class(BaseCase("", wo, ho, W, H, noc, l, wo * noc + extra, 0, offset)))
    return found


# ------------------------------------------------------------------ down: 2 x 2 means
# content: "u8" = 8-bit-derived (multiples of 1/16 below 256), "float" = arbitrary float32
DownCase = collections.namedtuple("DownCase", "w h noc content", defaults=("u8",))
DOWN_CASES = [DownCase(2, 2, 1), DownCase(3, 3, 1), DownCase(16, 6, 1), DownCase(7, 5, 3), DownCase(7, 5, 3, "float")]

# ------------------------------------------------------------------ planes: a level's image -> its padded planes (and `down`)
PlanesCase = collections.namedtuple("PlanesCase", "w h noc pad grad down content", defaults=("u8",))
PLANES_CASES = [
    # gray, quads
    PlanesCase(8, 2, 1, 4, True, False),      # every quad on the border path
    PlanesCase(12, 2, 1, 4, True, False),     # one vector-load quad
    PlanesCase(16, 6, 1, 4, True, True),      # fused down
    PlanesCase(16, 6, 1, 4, False, True),     # image B of a sequence: the lower row is fetched on even rows only
    PlanesCase(16, 6, 1, 4, False, False),    # neither gradients nor down
    PlanesCase(16, 5, 1, 8, True, True),      # odd h: down by a launch of its own -- and with it the generic planes kernel
    PlanesCase(64, 3, 1, 12, True, False),    # three workgroups per frame, the last one ragged
    PlanesCase(8, 2, 1, 4, True, True),       # fused down where no quad loads vectors
    PlanesCase(16, 6, 1, 4, True, True, "float"),
    # gray, generic
    PlanesCase(10, 7, 1, 4, True, False),     # w % 4 != 0 (two workgroups per frame, the last one ragged)
    PlanesCase(8, 4, 1, 6, True, False),      # pad % 4 != 0
    PlanesCase(4, 4, 1, 4, True, True),       # w < 8, and down by a launch of its own for gray
    PlanesCase(8, 1, 1, 4, True, False),      # h < 2 alone keeps a level off the quad kernel
    PlanesCase(2, 2, 1, 1, True, False),      # smallest two-sided level
    PlanesCase(1, 3, 1, 2, True, False),      # one-pixel width
    PlanesCase(3, 1, 1, 2, True, False),      # one-pixel height
    PlanesCase(10, 7, 1, 4, False, False),
    PlanesCase(10, 6, 1, 4, False, True),
    PlanesCase(10, 7, 1, 4, True, False, "float"),
    # RGB
    PlanesCase(5, 4, 3, 4, True, False),      # odd width
    PlanesCase(16, 6, 3, 12, True, True),     # down by a launch of its own
    PlanesCase(2, 2, 3, 1, True, False),      # smallest level
    PlanesCase(5, 4, 3, 4, False, False),     # image B of an RGB pair
    PlanesCase(6, 4, 3, 4, False, True),
]
PLANES_KERNELS = {0: "pyr_planes_kernel", 1: "pyr_planes_gray4_kernel", 2: "pyr_planes_gray4_kernel + down"}


def planes_class(c):
    """(kernel, noc, gradients, down): kernel 0 / 1 / 2 as pyr_planes_variant answers; down "no", "fused" (kernel 2) or
    "separate" (a pyr_down launch before kernel 0)"""
    variant = pyr_planes_variant(c.w, c.h, c.noc, c.pad, c.down)
    return variant, c.noc, bool(c.grad), ("fused" if variant == 2 else "separate") if c.down else "no"


def why_generic(c):
    """for a gray level on the generic planes kernel: the first condition of the quad kernel it misses"""
    if c.noc != 1 or pyr_planes_variant(c.w, c.h, c.noc, c.pad, c.down):
        return None
    for why, missed in (("w % 4", c.w % 4), ("pad % 4", c.pad % 4), ("w < 8", c.w < 8), ("h < 2", c.h < 2), ("odd h with down", c.down and c.h % 2)):
        if missed:
            return why
    raise AssertionError(f"{c}: nothing keeps this level off the quad kernel")


def vector_quads(c):
    """for the quad kernel: "none" / "some" of a row's quads load 16 bytes at once (x0 >= 1 and x0 + 4 <= w - 1)"""
    if not pyr_planes_variant(c.w, c.h, c.noc, c.pad, c.down):
        return None
    return "some" if any(x0 >= 1 and x0 + 4 <= c.w - 1 for x0 in range(0, c.w, 4)) else "none"


def planes_sweep():
    """the geometries whose classes the lists must cover: every small level, gray and RGB, with and without gradients and down
    (down only where the next level has pixels)"""
    for w, h, noc, pad, grad, dn in itertools.product((1, 2, 3, 4, 5, 8, 10, 12, 16, 64), range(1, 8), (1, 3), (1, 2, 4, 6, 8, 12),
                                                       (True, False), (True, False)):
        if not dn or (w >= 2 and h >= 2):
            yield PlanesCase(w, h, noc, pad, grad, dn)


def missing(cases, universe, key):
    """the classes (by `key`) of `universe` without a member in `cases`"""
    have = {key(c) for c in cases}
    return sorted((k for k in {key(c) for c in universe} if k is not None and k not in have), key=repr)


def table():
    """the markdown table of DESIGN.md: one row per class and the cases of tests/test_gpu_pyramid.py that run it"""
    rows = ["| launcher | kernel | channels | class | cases of `tests/test_gpu_pyramid.py` |", "|---|---|---|---|---|"]
    by = collections.defaultdict(list)
    for c in BASE_CASES:
        by[base_class(c)].append(c.name)
    for (variant, noc, word), names in sorted(by.items(), key=lambda kv: (kv[0][0] == 0, kv[0])):
        kernel = f"`pyr_base16_kernel<{variant}>`" if variant else "`pyr_base_kernel`"
        rows.append(f"| `launch_pyr_base` | {kernel} | {noc} | word path: {word} of the blocks | {', '.join(names)} |")
    rows.append(f"| `launch_pyr_down` | `pyr_down_kernel` | 1, 3 | | {', '.join(f'{c.w}x{c.h}x{c.noc} {c.content}' for c in DOWN_CASES)} |")
    by = collections.defaultdict(list)
    for c in PLANES_CASES:
        by[planes_class(c)].append(f"{c.w}x{c.h} pad {c.pad}" + ("" if c.content == "u8" else " " + c.content))
    for (variant, noc, grad, dn), names in sorted(by.items()):
        rows.append(f"| `launch_pyr_planes` | `{PLANES_KERNELS[variant]}` | {noc} | gradients: {'yes' if grad else 'no'}; down: {dn} | "
                    f"{', '.join(names)} |")
    return "\n".join(rows)


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tools")]
    print(table())
