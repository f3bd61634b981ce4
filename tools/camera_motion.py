"""The camera motion of a clip from Python: one global motion model per consecutive pair of frames, fitted on the device straight
from the level flows of a SEQUENCE | REVERSE batch context (ofdis_batch_global_motion, include/ofdis.h) -- a translation or a
6-parameter affine model by trimmed least squares, pixels that fail the forward-backward test left out.

    python tools/camera_motion.py [--rgb] [--op 1..4] [--fused] [--model affine|translation|projective] [--rounds 3] [--thresh 1.0]
                                  [--no-fb] [--labels STEM] img0 img1 ... imgN [out.csv]

Images load as for tools/flow_images.py; at least two, all of one size.  Writes one CSV line per pair -- a0,a1,a2,a3,a4,a5,
n_valid,n_inliers,status -- to out.csv (a last argument ending in .csv) or to standard output: u(x, y) = a0 + a1*(x - cx) +
a2*(y - cy), v(x, y) = a3 + a4*(x - cx) + a5*(y - cy) with (cx, cy) the image centre; the coefficients are printed with 17
significant digits (they read back to the same doubles); status 0 = affine, 1 = translation (asked for, or too few / collinear
pixels), 2 = no valid pixel.  --labels STEM also writes the label map of every pair as <STEM>_000.png ...: 0 = inlier (moves
with the camera), 127 = outlier (moves on its own), 255 = invalid.  --no-fb fits on every pixel with a finite flow (no
forward-backward test).  --fused selects the FMA / fast-reciprocal arithmetic contract for the flow (default: the exact one);
the fit does not depend on it.  --model projective fits the 8-parameter quadratic model of ofdis_batch_projective_motion
instead -- u = a0 + a1*xc + a2*yc + p*xc, v = a3 + a4*xc + a5*yc + p*yc with p = a6*xc + a7*yc, xc = x - cx, yc = y - cy -- and
writes a0,...,a7,n_valid,n_inliers,count per pair, count the number of parameters solved (8, or 6, 2, 0 where the pixels do
not determine eight).  Not here: stabilisation (warping frames along a smoothed camera path)."""
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

LABEL_GREY = np.array([0, 127, 255], np.uint8)  # GM_INLIER, GM_OUTLIER, GM_INVALID
# --model: the Batch methods of the fit and of the compensation, and what the fit takes beyond rounds and thresh
MODELS = {"affine": ("global_motion", "motion_compensate", dict(model=capi.GM_AFFINE)),
          "translation": ("global_motion", "motion_compensate", dict(model=capi.GM_TRANSLATION_ONLY)),
          "projective": ("projective_motion", "projective_compensate", {})}


def csv_line(model, stats):
    return ",".join([repr(float(a)) for a in model] + [str(int(v)) for v in stats])


def main(argv):
    rgb = fused = False
    fb = True
    op, model, rounds, thresh, labels = 2, "affine", 3, 1.0, None
    args = []
    it = iter(argv)
    a = ""
    try:
        for a in it:
            if a == "--rgb":
                rgb = True
            elif a == "--fused":
                fused = True
            elif a == "--no-fb":
                fb = False
            elif a == "--op":
                op = int(next(it))
            elif a == "--model":
                model = next(it)
            elif a == "--rounds":
                rounds = int(next(it))
            elif a == "--thresh":
                thresh = float(next(it))
            elif a == "--labels":
                labels = next(it)
            else:
                args.append(a)
    except (ValueError, StopIteration):
        sys.exit(f"{a}: a value is missing or is not a number")
    # every option is checked here, before the first device call
    if model not in MODELS:
        sys.exit("--model: affine, translation or projective")
    if not 1 <= rounds <= capi.GM_MAX_ROUNDS:
        sys.exit("--rounds: an integer in 1..%d" % capi.GM_MAX_ROUNDS)
    if not (math.isfinite(thresh) and thresh > 0.0):
        sys.exit("--thresh: a finite value > 0 (pixels)")
    out_csv = args.pop() if args and args[-1].lower().endswith(".csv") else None
    if len(args) < 2:
        sys.exit(__doc__)
    noc = 3 if rgb else 1
    frames = [load(path, noc) for path in args]
    if any(f.shape != frames[0].shape for f in frames):
        sys.exit("all images must have one size")
    clip = np.ascontiguousarray(np.stack(frames))
    n, h, w = len(frames) - 1, clip.shape[1], clip.shape[2]
    if max(w, h) > capi.GM_MAX_SIDE:
        sys.exit("images of at most %d pixels a side" % capi.GM_MAX_SIDE)
    capi.set_tuning(contract=1 if fused else 0)
    p = oppoint(op, w, h, noc=noc)
    p.width, p.height = padded_size(w, h, p.sc_f)
    b = capi.Batch(p, n, reverse=True, sequence=True)
    d = capi.Dev(clip)
    b.build_pyramids_u8_seq(d.ptr, w, h)
    b.run()
    fit, compensate, how = MODELS[model]
    models, stats = getattr(b, fit)(w, h, rounds=rounds, thresh=thresh, fb_check=fb, **how)
    label = getattr(b, compensate)(models, w, h, thresh=thresh, fb_check=fb, residual=False)[1] if labels else None
    b.close()
    d.free()
    lines = [csv_line(m, s) for m, s in zip(models, stats)]
    if out_csv:
        with open(out_csv, "w") as f:
            f.write("\n".join(lines) + "\n")
    else:
        print("\n".join(lines))
    if labels:
        from PIL import Image
        for k, lab in enumerate(label):
            Image.fromarray(LABEL_GREY[lab]).save(f"{labels}_{k:03d}.png")


if __name__ == "__main__":
    main(sys.argv[1:])
