"""A clip stabilised from Python through a SEQUENCE | REVERSE batch context: every frame held once, both flow directions of every
pair on the device, then ofdis_batch_stabilize (include/ofdis.h): one affine camera model per pair by trimmed least squares,
the motions relative to every frame averaged over a Gaussian window, and the frames resampled by the correcting warps.
--model projective takes ofdis_batch_stabilize_projective instead: 8-parameter models, the path chained on homographies, the
frames resampled by a perspective warp -- for pans and tilts, whose keystone an affine warp leaves at the corners.

    python tools/stabilize_frames.py [--model affine|projective] [--rgb] [--op 1..4] [--fused] [--radius 8] [--sigma 4.0]
                                     [--zoom 1.0] [--border constant|replicate] img0 img1 ... imgN out_stem

Images load as for tools/flow_images.py (B G R for --rgb, OpenCV's fixed-point BGR2GRAY otherwise); at least two, all of one
size.  Writes one PNG per frame, <out_stem>_000.png and so on (gray, or RGB converted back from B G R), and <out_stem>.csv with
one line per frame: the six numbers b0..b5 of its warp (out(x) = in(x + (b0 + b1*xc + b2*yc, b3 + b4*xc + b5*yc)), centred
coordinates; --model projective: the eight numbers g0..g7 of the map [[1+g1, g2, g0], [g4, 1+g5, g3], [-g6, -g7, 1]]), printed
with repr so that they read back bit for bit.  --radius / --sigma: the window, w_j = exp(-j^2 / (2
sigma^2)) for j = 0..radius (radius 0..64); --zoom in [1, 16] magnifies about the centre to hide the border a correction
exposes; --border: what the exposed border shows, zeros or the repeated edge.  --fused selects the FMA / fast-reciprocal
arithmetic contract for the flow (default: the exact one); the stabiliser itself does not depend on it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from flow_images import load  # noqa: E402
from of_dis_amd import capi, stabilize  # noqa: E402
from of_dis_amd.params import oppoint, padded_size  # noqa: E402


def main(argv):
    rgb = fused = False
    op, radius, sigma, zoom, border, model = 2, 8, 4.0, 1.0, "constant", "affine"
    args = []
    it = iter(argv)
    for a in it:
        if a == "--rgb":
            rgb = True
        elif a == "--fused":
            fused = True
        elif a == "--op":
            op = int(next(it))
        elif a == "--radius":
            radius = int(next(it))
        elif a == "--sigma":
            sigma = float(next(it))
        elif a == "--zoom":
            zoom = float(next(it))
        elif a == "--border":
            border = next(it)
        elif a == "--model":
            model = next(it)
        else:
            args.append(a)
    if len(args) < 3:
        sys.exit(__doc__)
    if border not in ("constant", "replicate"):
        sys.exit("--border: constant or replicate")
    if model not in ("affine", "projective"):
        sys.exit("--model: affine or projective")
    try:
        weights = stabilize.check_window(stabilize.gaussian_weights(radius, sigma), zoom)
    except ValueError as e:
        sys.exit(f"--radius / --sigma / --zoom: {e}")
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
    stabilise = b.stabilize_projective if model == "projective" else b.stabilize
    out, inside, warps = stabilise(d.ptr, w, h, weights, zoom=zoom,
                                   border=capi.BORDER_REPLICATE if border == "replicate" else capi.BORDER_CONSTANT,
                                   fb_check=True, inside=True)
    b.close()
    d.free()
    from PIL import Image
    with open(stem + ".csv", "w") as f:
        for k, (frame, ins, wp) in enumerate(zip(out, inside, warps)):
            path = f"{stem}_{k:03d}.png"
            Image.fromarray(np.ascontiguousarray(frame[..., ::-1]) if rgb else frame).save(path)
            f.write(",".join(repr(float(v)) for v in wp) + "\n")
            print(f"{path}: {w}x{h}, shift ({wp[0]:+.3f}, {wp[3]:+.3f}) px, covered {np.mean(ins):.3f} of the pixels")


if __name__ == "__main__":
    main(sys.argv[1:])
