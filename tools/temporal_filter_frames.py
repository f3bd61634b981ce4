"""A clip denoised from Python by motion-compensated temporal filtering, through a SEQUENCE | REVERSE batch context: every frame
held once, both flow directions of every pair on the device, then ofdis_batch_temporal_filter straight from the level flows
(include/ofdis.h): frame k averaged with frames k-1 and k+1 warped onto it, occluded pixels left out.  With --radius R > 1,
ofdis_batch_trajectory_filter: frame k averaged with the R frames before and the R frames after it, each sampled where the
pixel's trajectory through the flows of consecutive pairs stands in it.

    python tools/temporal_filter_frames.py [--rgb] [--op 1..4] [--fused] [--wn 1.0] [--tau inf] [--radius 1] [--sigma S]
                                           img0 img1 ... imgN out_stem

Images load as for tools/flow_images.py (B G R for --rgb, OpenCV's fixed-point BGR2GRAY otherwise); at least two, all of one
size.  Writes one PNG per frame, <out_stem>_000.png and so on (gray, or RGB converted back from B G R), and prints per frame
the share of pixels averaged with both neighbours, with one and with none.  --wn: the neighbour strength in [0, 1]; --tau: the
photometric gate in grey levels (a neighbour that differs by tau or more gets weight 0; inf: no gate).  --radius: 1..8 frames
on either side (1: the three-frame filter, the same call and bytes as without the option); --sigma: frame j steps away weighs
wn * exp(-j^2 / (2 S^2)) instead of wn (only with --radius above 1).  --fused selects the
FMA / fast-reciprocal arithmetic contract for the flow (default: the exact one); the filter does not depend on it."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from flow_images import load  # noqa: E402
from of_dis_amd import capi  # noqa: E402
from of_dis_amd.params import oppoint, padded_size  # noqa: E402
from of_dis_amd.temporal import reach, trajectory_weights  # noqa: E402


def main(argv):
    rgb = fused = False
    op, wn, tau, radius, sigma = 2, 1.0, math.inf, 1, None
    args = []
    it = iter(argv)
    for a in it:
        if a == "--rgb":
            rgb = True
        elif a == "--fused":
            fused = True
        elif a == "--op":
            op = int(next(it))
        elif a == "--wn":
            wn = float(next(it))
        elif a == "--tau":
            tau = float(next(it))
        elif a == "--radius":
            radius = int(next(it))
        elif a == "--sigma":
            sigma = float(next(it))
        else:
            args.append(a)
    if len(args) < 3:
        sys.exit(__doc__)
    if not 0.0 <= wn <= 1.0:
        sys.exit("--wn: a value in [0, 1]")
    if not tau >= float(np.finfo(np.float32).tiny):
        sys.exit("--tau: inf or a positive (normal) float")
    if not 1 <= radius <= capi.TRAJ_MAX_RADIUS:
        sys.exit(f"--radius: 1..{capi.TRAJ_MAX_RADIUS}")
    if sigma is not None and (radius == 1 or not sigma > 0.0):
        sys.exit("--sigma: a positive value, with --radius above 1")
    noc = 3 if rgb else 1
    frames, stem = [load(path, noc) for path in args[:-1]], args[-1]
    if any(f.shape != frames[0].shape for f in frames):
        sys.exit("all images must have one size")
    clip = np.ascontiguousarray(np.stack(frames))
    n, h, w = len(frames) - 1, clip.shape[1], clip.shape[2]
    capi.set_tuning(contract=1 if fused else 0)
    p = oppoint(op, w, h, noc=noc)
    p.width, p.height = padded_size(w, h, p.sc_f)
    b = capi.Batch(p, n, reverse=True, sequence=True)
    d = capi.Dev(clip)
    b.build_pyramids_u8_seq(d.ptr, w, h)
    b.run()
    if radius == 1:
        out, support = b.temporal_filter(d.ptr, w, h, wn=wn, tau=tau, support=True)
    else:
        out, support = b.trajectory_filter(d.ptr, w, h, trajectory_weights(radius, wn, sigma), tau=tau, support=True)
    b.close()
    d.free()
    from PIL import Image
    for k, (frame, sup) in enumerate(zip(out, support)):
        path = f"{stem}_{k:03d}.png"
        Image.fromarray(np.ascontiguousarray(frame[..., ::-1]) if rgb else frame).save(path)
        if radius > 1:
            nb, nf = reach(sup)
            print(f"{path}: {w}x{h}, frames averaged per pixel: {1 + nb.mean() + nf.mean():.2f} of {2 * radius + 1}, "
                  f"full reach at {np.mean((nb == radius) & (nf == radius)):.3f} of the pixels")
            continue
        print(f"{path}: {w}x{h}, neighbours: both {np.mean(sup == 3):.3f}, one {np.mean((sup == 1) | (sup == 2)):.3f}, "
              f"none {np.mean(sup == 0):.3f} of the pixels")


if __name__ == "__main__":
    main(sys.argv[1:])
