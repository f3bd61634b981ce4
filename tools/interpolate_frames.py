"""In-between frames of an image pair from Python, through a REVERSE batch context: both flow directions on the device,
then ofdis_batch_interpolate straight from the level flows (include/ofdis.h).  The masks are written separately, only for
the printed fractions.

    python tools/interpolate_frames.py [--rgb] [--op 1..4] [--fused] [--times 0.25,0.5,0.75] imgA imgB out_stem

Images load as for tools/flow_images.py (B G R for --rgb, OpenCV's fixed-point BGR2GRAY otherwise).  Writes one PNG per time,
<out_stem>.t0.500.png and so on (gray, or RGB converted back from B G R), and prints the consistent fraction of each
direction's mask (ofdis_batch_upsample_bidir with the default alpha 0.01 and beta 0.5).  --fused selects the FMA /
fast-reciprocal arithmetic contract for the flow (default: the exact one); the interpolation does not depend on it.
Default times: 0.5."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from flow_images import load  # noqa: E402
from of_dis_amd import capi  # noqa: E402
from of_dis_amd.params import oppoint, padded_size  # noqa: E402


def main(argv):
    rgb = fused = False
    op, times = 2, [0.5]
    args = []
    it = iter(argv)
    for a in it:
        if a == "--rgb":
            rgb = True
        elif a == "--fused":
            fused = True
        elif a == "--op":
            op = int(next(it))
        elif a == "--times":
            times = [float(x) for x in next(it).split(",") if x]
        else:
            args.append(a)
    if len(args) != 3:
        sys.exit(__doc__)
    if not 1 <= len(times) <= capi.INTERP_MAX_TIMES or not all(0.0 <= t <= 1.0 for t in times):
        sys.exit(f"--times: 1..{capi.INTERP_MAX_TIMES} values in [0, 1]")
    noc = 3 if rgb else 1
    a, b_, stem = load(args[0], noc), load(args[1], noc), args[2]
    if a.shape != b_.shape:
        sys.exit("both images must have one size")
    h, w = a.shape[:2]
    capi.set_tuning(contract=1 if fused else 0)
    p = oppoint(op, w, h, noc=noc)
    p.width, p.height = padded_size(w, h, p.sc_f)
    b = capi.Batch(p, 1, reverse=True)
    da, db = capi.Dev(a[None]), capi.Dev(b_[None])
    b.build_pyramids_u8(da.ptr, db.ptr, w, h)
    b.run()
    out = b.interpolate(da.ptr, db.ptr, w, h, times)[0]
    _, _, mask_fw, mask_rev = b.upsample_bidir(w, h, outputs=(False, False, True, True))
    b.close()
    da.free()
    db.free()
    from PIL import Image
    for t, frame in zip(times, out):
        path = f"{stem}.t{t:.3f}.png"
        Image.fromarray(np.ascontiguousarray(frame[..., ::-1]) if rgb else frame).save(path)
        print(f"{path}: {w}x{h}, t = {t}")
    print(f"consistent: {np.mean(mask_fw[0] == 0):.3f} of the pixels A -> B, {np.mean(mask_rev[0] == 0):.3f} B -> A")


if __name__ == "__main__":
    main(sys.argv[1:])
