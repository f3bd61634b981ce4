"""Video stabilisation of a sequence context, stage by stage: ofdis_batch_global_motion (the models, from the level flows),
ofdis_camera_path (one warp per frame) and ofdis_warp_frames (the frames resampled), then ofdis_batch_stabilize, which is the
three in one call, and the bytes the warp kernel moves against the time it takes.  Then the projective route on the same
context, in the same job: ofdis_batch_projective_motion, ofdis_camera_path_projective, ofdis_warp_frames_projective and
ofdis_batch_stabilize_projective, one row each beside the affine one.

1024x436, gray and RGB, operating point 2, TV on, fused arithmetic contract for the flow passes (the stabilisation kernels are
independent of the contract), one GPU, an OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE context of 1024 pairs over the clip of
tools/track_probe.py (one texture in slow periodic motion; RGB: the same plane three times).  Affine model, 3 rounds, thresh 1,
fb_check = 1; Gaussian window of radius 16 and sigma 8, zoom 1.05, OFDIS_BORDER_CONSTANT, `inside` written.  HIP events on one
non-default stream, warm-up first, the stages timed alternately in several rounds; the median round is reported.  The warp
kernel's bytes are the algorithmic ones -- every frame read once, `out` and `inside` written once -- and the fraction is of
bench.HBM_PEAK_GBS.  Bit equality of the one call with the three is checked on out, inside and the warps.

    python tools/stabilize_probe.py [--pairs 1024] [--out profiles/stabilize_probe.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench  # noqa: E402
from of_dis_amd import capi, stabilize  # noqa: E402
from of_dis_amd.params import oppoint  # noqa: E402
from track_probe import H, W, alternate, clip  # noqa: E402

MODEL, ROUNDS, THRESH = capi.GM_AFFINE, 3, 1.0
RADIUS, SIGMA, ZOOM, BORDER = 16, 8.0, 1.05, capi.BORDER_CONSTANT


def measure(frames, noc, tstream, dev, rounds, steps):
    """frames: [n + 1][H][W] (gray) or [n + 1][H][W][3] u8 on the device; returns the affine row and the projective row"""
    s = tstream.cuda_stream
    n = frames.shape[0] - 1
    p = oppoint(2, W, H, noc=noc, usetvref=1, verbosity=0)
    b = capi.Batch(p, n, reverse=True, sequence=True)
    b.build_pyramids_u8_seq(frames.data_ptr(), W, H, stream=s)
    b.run(s)
    b.join(s)
    tstream.synchronize()
    if b.status() != 0:
        raise SystemExit("the pass failed (ofdis_batch_status)")
    weights = stabilize.gaussian_weights(RADIUS, SIGMA)
    rows = [route(b, frames, noc, tstream, dev, rounds, steps, weights, nparam) for nparam in (6, 8)]
    b.close()
    return rows


def route(b, frames, noc, tstream, dev, rounds, steps, weights, nparam):
    """the three stages and the one call of the affine (nparam = 6) or the projective (8) route on the context b"""
    L = capi.lib()
    s = tstream.cuda_stream
    n = frames.shape[0] - 1
    before = b.device_bytes()
    wp = weights.ctypes.data
    models = torch.empty((n, nparam), dtype=torch.float64, device=dev)
    warps = [torch.empty((n + 1, nparam), dtype=torch.float64, device=dev) for _ in range(2)]
    out = [torch.empty_like(frames) for _ in range(2)]
    inside = [torch.empty((n + 1, H, W), dtype=torch.uint8, device=dev) for _ in range(2)]
    a, be = capi.FB_ALPHA, capi.FB_BETA
    fp, o0, o1, i0, i1 = frames.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), inside[0].data_ptr(), inside[1].data_ptr()
    mp, w0, w1 = models.data_ptr(), warps[0].data_ptr(), warps[1].data_ptr()

    if nparam == 6:
        def fit():
            capi.check(L.ofdis_batch_global_motion(b.h, 0, n, MODEL, ROUNDS, THRESH, 1, a, be, mp, None, W, H, s))

        def path():
            capi.check(L.ofdis_camera_path(mp, n, wp, RADIUS, ZOOM, w0, s))

        def warp():
            capi.check(L.ofdis_warp_frames(fp, w0, o0, i0, n + 1, W, H, noc, BORDER, s))

        def whole():
            capi.check(L.ofdis_batch_stabilize(b.h, fp, 0, n, MODEL, ROUNDS, THRESH, 1, a, be, wp, RADIUS, ZOOM, BORDER, o1, i1, w1,
                                               W, H, s))
    else:
        def fit():
            capi.check(L.ofdis_batch_projective_motion(b.h, 0, n, ROUNDS, THRESH, 1, a, be, mp, None, W, H, s))

        def path():
            capi.check(L.ofdis_camera_path_projective(mp, n, W, H, wp, RADIUS, ZOOM, w0, s))

        def warp():
            capi.check(L.ofdis_warp_frames_projective(fp, w0, o0, i0, n + 1, W, H, noc, BORDER, s))

        def whole():
            capi.check(L.ofdis_batch_stabilize_projective(b.h, fp, 0, n, ROUNDS, THRESH, 1, a, be, wp, RADIUS, ZOOM, BORDER, o1,
                                                          i1, w1, W, H, s))

    t_fit, t_path, t_warp, t_whole = alternate(tstream, [fit, path, warp, whole], rounds, steps, 2)
    tstream.synchronize()
    equal = bool(torch.equal(warps[0].view(torch.int64), warps[1].view(torch.int64)) and torch.equal(out[0], out[1])
                 and torch.equal(inside[0], inside[1]))
    med = statistics.median
    px = (n + 1) * W * H
    warp_bytes = px * (2 * noc + 1)      # the frame read once, out and inside written once
    gbs = warp_bytes / (med(t_warp) * 1e-3) / 1e9
    names = (("global_motion", "camera_path", "warp_frames", "batch_stabilize") if nparam == 6 else
             ("projective_motion", "camera_path_projective", "warp_frames_projective", "batch_stabilize_projective"))
    r = {"noc": noc, "pairs": n, "model": "affine" if nparam == 6 else "projective", "rounds": ROUNDS, "thresh": THRESH,
         "radius": RADIUS, "sigma": SIGMA, "zoom": ZOOM, "border": "constant",
         names[0] + "_ms": round(med(t_fit), 4), names[1] + "_ms": round(med(t_path), 4), names[2] + "_ms": round(med(t_warp), 4),
         names[3] + "_ms": round(med(t_whole), 4), "frames_per_s": round((n + 1) / (med(t_whole) * 1e-3)),
         "warp_bytes": warp_bytes, "warp_bytes_per_pixel": 2 * noc + 1, "warp_GBs": round(gbs, 1),
         "warp_frac_of_hbm_peak": round(gbs / bench.HBM_PEAK_GBS, 4),
         "context_scratch_bytes": b.device_bytes() - before,
         "inside_share": round(float(inside[0].float().mean()), 4),
         "largest_shift_px": round(float(warps[0][:, [0, 3]].abs().max()), 4),
         "one_call_equals_three": equal,
         "rounds_ms": {names[0]: [round(x, 4) for x in t_fit], names[1]: [round(x, 4) for x in t_path],
                       names[2]: [round(x, 4) for x in t_warp], names[3]: [round(x, 4) for x in t_whole]}}
    if nparam == 8:
        r["largest_perspective_term"] = float(warps[0][:, 6:].abs().max())
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stabilize_probe.py measures on a GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    capi.check(capi.lib().ofdis_set_device(0))
    gray = clip(args.pairs + 1, dev)
    tstream = torch.cuda.Stream(device=dev)
    old = capi.set_tuning(contract=1)
    rows = []
    try:
        rows += measure(gray, 1, tstream, dev, args.rounds, args.steps)
        rgb = gray[..., None].expand(-1, -1, -1, 3).contiguous()
        del gray
        rows += measure(rgb, 3, tstream, dev, args.rounds, args.steps)
    finally:
        capi.restore_tuning(old)
    doc = {"tool": "tools/stabilize_probe.py", "build_id": capi.build_id(), "device": torch.cuda.get_device_name(0),
           "geometry": f"{W}x{H}, operating point 2, TV on, fused contract for the flow, SEQUENCE | REVERSE context, one texture in "
                       f"periodic motion of at most ~1.2 px per pair; affine and projective, {ROUNDS} rounds, thresh {THRESH}, fb_check = 1; "
                       f"Gaussian window radius {RADIUS} sigma {SIGMA}, zoom {ZOOM}, constant border, inside written",
           "basis": "HIP events on one stream, warm-up, the stages timed alternately per round, median round; warp_bytes = "
                    "(frames + 1) * W * H * (2 * noc + 1): every frame read once, out and inside written once; "
                    f"warp_frac_of_hbm_peak against {bench.HBM_PEAK_GBS} GB/s",
           "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "rows"}))


if __name__ == "__main__":
    main()
