"""Global motion models of a sequence context: ofdis_batch_global_motion + ofdis_batch_motion_compensate (fused: flows and codes
straight from the level flows) against the materialised route (ofdis_batch_upsample_bidir for all pairs -- forward flow and
forward mask -- then ofdis_global_motion and ofdis_motion_compensate on its two arrays; its time includes that upsample), and
the bytes each route writes.

1024x436 gray, operating point 2, TV on, fused arithmetic contract for the flow passes (the global-motion kernels are
independent of the contract), one GPU, an OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE context of 1024 pairs over the clip of
tools/track_probe.py (one texture in slow periodic motion).  Affine model, 3 rounds, thresh 1, fb_check = 1; compensate writes
the labels only (the background / foreground split: the residual flow is 8 bytes per pixel on either route).  HIP events on
one non-default stream, warm-up first, the routes timed alternately in several rounds; the median round is reported.  Bit
equality of the two routes is checked on the models, the stats and the labels.

    python tools/gmotion_probe.py [--pairs 1024] [--out profiles/gmotion_probe.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from of_dis_amd import capi  # noqa: E402
from of_dis_amd.params import oppoint  # noqa: E402
from track_probe import H, W, alternate, clip  # noqa: E402

MODEL, ROUNDS, THRESH = capi.GM_AFFINE, 3, 1.0


def measure(frames, tstream, dev, rounds, steps):
    """frames: [n + 1][H][W] u8 on the device"""
    L = capi.lib()
    s = tstream.cuda_stream
    n = frames.shape[0] - 1
    p = oppoint(2, W, H, noc=1, usetvref=1, verbosity=0)
    b = capi.Batch(p, n, reverse=True, sequence=True)
    b.build_pyramids_u8_seq(frames.data_ptr(), W, H, stream=s)
    b.run(s)
    b.join(s)
    tstream.synchronize()
    if b.status() != 0:
        raise SystemExit("the pass failed (ofdis_batch_status)")
    before = b.device_bytes()
    models = [torch.empty((n, 6), dtype=torch.float64, device=dev) for _ in range(2)]
    stats = [torch.empty((n, 3), dtype=torch.int64, device=dev) for _ in range(2)]
    label = [torch.empty((n, H, W), dtype=torch.uint8, device=dev) for _ in range(2)]
    fw = torch.empty((n, H, W, 2), dtype=torch.float32, device=dev)
    mf = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    work_bytes = L.ofdis_global_motion_work_bytes(n, W, H)
    work = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
    a, be = capi.FB_ALPHA, capi.FB_BETA

    def fused_fit():
        capi.check(L.ofdis_batch_global_motion(b.h, 0, n, MODEL, ROUNDS, THRESH, 1, a, be, models[0].data_ptr(),
                                               stats[0].data_ptr(), W, H, s))

    def fused():
        fused_fit()
        capi.check(L.ofdis_batch_motion_compensate(b.h, 0, n, models[0].data_ptr(), THRESH, 1, a, be, None, label[0].data_ptr(), W,
                                                   H, s))

    def upsample():
        capi.check(L.ofdis_batch_upsample_bidir(b.h, 0, n, fw.data_ptr(), None, mf.data_ptr(), None, W, H, a, be, s))

    def standalone_fit():
        capi.check(L.ofdis_global_motion(fw.data_ptr(), mf.data_ptr(), n, W, H, MODEL, ROUNDS, THRESH, models[1].data_ptr(),
                                         stats[1].data_ptr(), work.data_ptr(), work_bytes, s))

    def materialised():
        upsample()
        standalone_fit()
        capi.check(L.ofdis_motion_compensate(fw.data_ptr(), mf.data_ptr(), models[1].data_ptr(), n, W, H, THRESH, None,
                                             label[1].data_ptr(), s))

    t_f, t_m, t_ff, t_sf = alternate(tstream, [fused, materialised, fused_fit, standalone_fit], rounds, steps, 2)
    tstream.synchronize()
    equal = bool(torch.equal(models[0].view(torch.int64), models[1].view(torch.int64)) and torch.equal(stats[0], stats[1])
                 and torch.equal(label[0], label[1]))
    med = statistics.median
    px = W * H
    small = n * (48 + 24)        # models + stats
    r = {"pairs": n, "model": "affine", "rounds": ROUNDS, "thresh": THRESH,
         "fused_ms": round(med(t_f), 4), "materialised_ms": round(med(t_m), 4),
         "fused_fit_only_ms": round(med(t_ff), 4), "materialised_fit_kernels_only_ms": round(med(t_sf), 4),
         "materialised_over_fused": round(med(t_m) / med(t_f), 3),
         "faster": "fused" if med(t_f) < med(t_m) else "materialised",
         "fused_pairs_per_s": round(n / (med(t_f) * 1e-3)),
         "bytes_written": {"fused": small + n * px + ROUNDS * work_bytes,
                           "materialised": small + n * px + ROUNDS * work_bytes + n * px * 9},
         "slab_bytes": work_bytes, "context_scratch_bytes": b.device_bytes() - before,
         "valid_share": round(float(stats[0][:, 0].double().mean()) / px, 4),
         "inlier_share_of_valid": round(float((stats[0][:, 1].double() / stats[0][:, 0].clamp(min=1).double()).mean()), 4),
         "status_counts": [int((stats[0][:, 2] == k).sum()) for k in range(3)],
         "routes_bit_equal": equal,
         "rounds_ms": {"fused": [round(x, 4) for x in t_f], "materialised": [round(x, 4) for x in t_m],
                       "fused_fit_only": [round(x, 4) for x in t_ff],
                       "materialised_fit_kernels_only": [round(x, 4) for x in t_sf]}}
    print(json.dumps(r), flush=True)
    b.close()
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gmotion_probe.py measures on a GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    capi.check(capi.lib().ofdis_set_device(0))
    gray = clip(args.pairs + 1, dev)
    tstream = torch.cuda.Stream(device=dev)
    old = capi.set_tuning(contract=1)
    try:
        row = measure(gray, tstream, dev, args.rounds, args.steps)
    finally:
        capi.restore_tuning(old)
    doc = {"tool": "tools/gmotion_probe.py", "build_id": capi.build_id(), "device": torch.cuda.get_device_name(0),
           "geometry": f"{W}x{H} gray, operating point 2, TV on, fused contract for the flow, SEQUENCE | REVERSE context, one "
                       f"texture in periodic motion of at most ~1.2 px per pair; affine, {ROUNDS} rounds, thresh {THRESH}, "
                       "fb_check = 1, labels written",
           "basis": "HIP events on one stream, warm-up, the routes timed alternately per round, median round; fused = "
                    "ofdis_batch_global_motion + ofdis_batch_motion_compensate; materialised = ofdis_batch_upsample_bidir (forward "
                    "flow and mask: 9 bytes per pixel and pair) + ofdis_global_motion + ofdis_motion_compensate; bytes_written = "
                    "models + stats + labels + the slab once per round (+ those arrays)",
           "rows": [row]}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "rows"}))


if __name__ == "__main__":
    main()
