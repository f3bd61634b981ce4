"""Which patch kernel launch_patch_optimize runs (choose_patch_kernel, ofdis_kernels.h), on the host (no GPU).

Under the exact contract every patch kernel gives the same bits, so a level that silently takes the wrong one passes every
bit-exact test.  The choice is a pure host function; here it is held, over the whole table of geometries, modes, cost
functions, knobs and contracts, against an independent restatement of the ladder the launcher held before the choice became
a function of its own (reference_ladder below: it stays as it is, it is the reference).  patch_pixel_weights_supported is the
choice's `pixw`: true exactly where the kernel is one of the two 16-lane RGB 12x12 flow kernels.
"""
import itertools

import pytest

from launch_hooks import patch_kernel_choice

GEOMETRIES = [(8, 1), (8, 3), (12, 1), (12, 3), (16, 1), (16, 3), (20, 1), (24, 3)]   # (P, noc); the last one is refused
# patches per level: 40 leave the gray 8x8 kernel fewer than four wavefronts per frame (its workgroup shrinks), 1000 do not
NOPS = [1, 40, 1000]
TABLE = list(itertools.product(GEOMETRIES, [0, 1], [0, 1, 2], [0, 1], [0, 1], [0, 16, 32, 64], [0, 1]))


def reference_ladder(P, noc, nop, stereo, costfct, pixw, gray8_knob, rgb12_knob, lpp_knob, contract):
    """(kernel instantiation as written in the source, workgroup size, workgroups per frame), or None where the launcher
    refuses: the if / else-if ladder of launch_patch_optimize and launch_patch_optimize_rgb12, restated line by line"""
    novals = noc * P * P
    M = (novals + 63) // 64
    full = novals == 64 * M
    gray8 = noc == 1 and P == 8 and bool(gray8_knob)
    rgb12_lpp = 16 if lpp_knob == 0 else lpp_knob
    rgb12 = novals == 432 and not stereo and costfct in (0, 1) and bool(rgb12_knob)
    p12 = ((P == 12 and noc in (1, 3)) or (P == 8 and noc == 3)) and costfct in (0, 1) and bool(rgb12_knob)
    if p12 and rgb12_lpp == 16:
        wpf = (nop + 3) // 4
        kernel = "patch_optimize_rgb12_kernel" if contract else "patch_optimize_rgb12x_kernel"
        l1 = 1 if costfct != 0 else 0
        st = "true" if stereo else "false"
        if P == 8:
            targs = f"<{l1}, 3, {st}, 2>"
        elif noc == 1:
            targs = f"<{l1}, 1, {st}, 3>"
        else:
            targs = f"<{l1}, 3, {st}, 3>"
        return kernel + targs, 256, (wpf + 3) // 4
    if pixw:
        return None
    lpp = (4 if gray8 else 8) if M <= 1 else (32 if (rgb12 and rgb12_lpp == 32) else 64)
    ppw = 64 // lpp
    wpf = (nop + ppw - 1) // ppw
    fast = gray8 and M <= 1
    wpb = wpf if (fast and wpf < 4) else 4
    geometry = (wpb * 64, (wpf + wpb - 1) // wpb)
    if M <= 1 and gray8 and stereo:
        name = "patch_optimize_gray8_kernel<-1, true>"
    elif M <= 1 and gray8 and costfct == 0:
        name = "patch_optimize_gray8_kernel<0, false>"
    elif M <= 1 and gray8:
        name = "patch_optimize_gray8_kernel<-1, false>"
    elif M <= 1 and full and costfct == 0:
        name = "patch_optimize_kernel<1, 8, 64, 0>"
    elif M <= 1 and full:
        name = "patch_optimize_kernel<1, 8, 64, -1>"
    elif M <= 1:
        name = "patch_optimize_kernel<1, 8, 0, -1>"
    elif M <= 3:
        name = "patch_optimize_kernel<3, 64, 0, -1>"
    elif rgb12 and lpp == 32 and costfct == 0:
        name = "patch_optimize_kernel<7, 32, 432, 0>"
    elif rgb12 and lpp == 32:
        name = "patch_optimize_kernel<7, 32, 432, 1>"
    elif rgb12 and costfct == 0:
        name = "patch_optimize_kernel<7, 64, 432, 0>"
    elif rgb12:
        name = "patch_optimize_kernel<7, 64, 432, 1>"
    elif M <= 7:
        name = "patch_optimize_kernel<7, 64, 0, -1>"
    elif M <= 12:
        name = "patch_optimize_kernel<12, 64, 0, -1>"
    else:
        return None
    return (name,) + geometry


def reference_pixel_weights_supported(P, noc, stereo, costfct, rgb12_knob, lpp_knob):
    """patch_pixel_weights_supported as it was written by hand beside the ladder"""
    return noc * P * P == 432 and P == 12 and not stereo and costfct in (0, 1) and bool(rgb12_knob) and (lpp_knob or 16) == 16


def chosen(c, contract):
    """the choice in the form of reference_ladder"""
    if c["family"] == "none":
        return None
    t = c["targs"]
    b = ("false", "true")
    if c["family"] == "lanes16":
        name = ("patch_optimize_rgb12_kernel" if contract else "patch_optimize_rgb12x_kernel") + f"<{t[0]}, {t[1]}, {b[t[2]]}, {t[3]}>"
    elif c["family"] == "gray8":
        name = f"patch_optimize_gray8_kernel<{t[0]}, {b[t[1]]}>"
    else:
        name = f"patch_optimize_kernel<{t[0]}, {t[1]}, {t[2]}, {t[3]}>"
    return name, c["threads"], c["blocks_per_frame"]


PIXW_KERNELS = {f"patch_optimize_rgb12{x}_kernel<{l1}, 3, false, 3>" for x in ("", "x") for l1 in (0, 1)}


@pytest.mark.parametrize("pixw_asked", [0, 1], ids=["no-pixw", "pixw-asked"])
def test_choice_is_the_ladder_over_the_whole_table(pixw_asked):
    seen = set()
    for (P, noc), stereo, costfct, gray8, rgb12, lpp, contract in TABLE:
        for nop in NOPS:
            what = f"P {P} noc {noc} nop {nop} stereo {stereo} costfct {costfct} gray8 {gray8} rgb12 {rgb12} lpp {lpp} contract {contract}"
            c = patch_kernel_choice(P, noc, nop, stereo, costfct, pixw_asked, gray8, rgb12, lpp, contract)
            want = reference_ladder(P, noc, nop, stereo, costfct, pixw_asked, gray8, rgb12, lpp, contract)
            got = chosen(c, contract)
            assert got == want, what
            if (P, noc) == (24, 3):
                assert got is None, what
            # the lanes per patch the grid was made from are the kernel's own
            if c["family"] == "generic":
                assert c["lpp"] == c["targs"][1], what
            elif got:
                assert c["lpp"] == {"lanes16": 16, "gray8": 4}[c["family"]], what
            # the compact per-pixel weights: as the hand-written rule had it, and exactly with the two kernels that write them
            assert c["pixw"] == reference_pixel_weights_supported(P, noc, stereo, costfct, rgb12, lpp), what
            assert c["pixw"] == (got is not None and got[0] in PIXW_KERNELS), what
            if got:
                seen.add(got[0])
    # the table reaches every instantiation there is -- the 12 of either contract's 16-lane kernel, the 3 gray 8x8, 9 of the 10
    # generic ones -- but patch_optimize_kernel<1, 8, 0, -1> (fewer than 64 values per patch: no such geometry in it); with the
    # pixel weights asked for, every kernel but the 16-lane ones is refused
    assert len(seen) == (24 if pixw_asked else 24 + 3 + 9), sorted(seen)


def test_pixel_weights_question_does_not_depend_on_the_request():
    """patch_pixel_weights_supported asks with the weights requested; the answer is the same without"""
    for (P, noc), stereo, costfct, gray8, rgb12, lpp, contract in TABLE:
        a = patch_kernel_choice(P, noc, 1000, stereo, costfct, 0, gray8, rgb12, lpp, contract)
        b = patch_kernel_choice(P, noc, 1000, stereo, costfct, 1, gray8, rgb12, lpp, contract)
        assert a["pixw"] == b["pixw"]
        if a["pixw"]:
            assert a == b
