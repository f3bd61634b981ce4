"""Temporal filtering along flow trajectories on a sequence context: ofdis_batch_trajectory_filter (fused: the flows straight from
the level flows) against the materialised route (ofdis_batch_upsample_bidir for all pairs -- both flows, no masks -- then
ofdis_trajectory_filter on them; its time includes that upsample), at radius 1, 2 and 4, and the bytes each route writes.  At
radius 1 the existing three-frame ofdis_batch_temporal_filter is timed next to them and its out compared: a figure to report,
not a requirement.

1024x436, gray and RGB, operating point 2, TV on, fused arithmetic contract for the flow passes (the filter kernels are
independent of the contract), one GPU, an OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE context of 1024 pairs over the clip of
tools/track_probe.py (one texture in slow periodic motion; RGB: three grey-level maps of it).  Flat weights 1, tau = 24,
fb_check = 1, support written.  HIP events on one non-default stream, warm-up first, the routes timed alternately in several
rounds; the median round is reported.  Bit equality of the routes is checked on the whole out and support arrays.

    python tools/trajfilter_probe.py [--pairs 1024] [--out profiles/trajfilter_probe.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from of_dis_amd import capi  # noqa: E402
from of_dis_amd.params import oppoint  # noqa: E402
from track_probe import H, W, alternate, clip  # noqa: E402

TAU = 24.0
RADII = (1, 2, 4)


def measure(frames, noc, tstream, dev, rounds, steps):
    """frames: [n + 1][H][W] (+ [3]) u8 on the device; one row per radius"""
    L = capi.lib()
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
    out = [torch.empty_like(frames) for _ in range(3)]
    sup = [torch.empty((n + 1, H, W), dtype=torch.uint8, device=dev) for _ in range(3)]
    fw = torch.empty((n, H, W, 2), dtype=torch.float32, device=dev)
    rv = torch.empty_like(fw)
    px = W * H
    out_bytes = (n + 1) * px * (noc + 1)
    med = statistics.median
    rows = []
    for radius in RADII:
        wts = np.ones(radius, np.float32)
        wp = wts.ctypes.data

        def fused():
            capi.check(L.ofdis_batch_trajectory_filter(b.h, frames.data_ptr(), 0, n, out[0].data_ptr(), sup[0].data_ptr(), W, H,
                                                       wp, radius, TAU, 1, capi.FB_ALPHA, capi.FB_BETA, s))

        def standalone():
            capi.check(L.ofdis_trajectory_filter(frames.data_ptr(), fw.data_ptr(), rv.data_ptr(), out[1].data_ptr(),
                                                 sup[1].data_ptr(), n, W, H, noc, wp, radius, TAU, 1, capi.FB_ALPHA,
                                                 capi.FB_BETA, s))

        def materialised():
            capi.check(L.ofdis_batch_upsample_bidir(b.h, 0, n, fw.data_ptr(), rv.data_ptr(), None, None, W, H, capi.FB_ALPHA,
                                                    capi.FB_BETA, s))
            standalone()

        def three_frames():
            capi.check(L.ofdis_batch_temporal_filter(b.h, frames.data_ptr(), 0, n, out[2].data_ptr(), sup[2].data_ptr(), W, H,
                                                     1.0, TAU, capi.FB_ALPHA, capi.FB_BETA, s))

        fns = [fused, materialised, standalone] + ([three_frames] if radius == 1 else [])
        times = alternate(tstream, fns, rounds, steps, 2)
        tstream.synchronize()
        t_f, t_m, t_s = times[:3]
        nb, nf = sup[0][radius:n + 1 - radius] >> 4, sup[0][radius:n + 1 - radius] & 15
        r = {"channels": noc, "pairs": n, "radius": radius,
             "fused_ms": round(med(t_f), 4), "materialised_ms": round(med(t_m), 4),
             "materialised_filter_kernel_ms": round(med(t_s), 4),
             "materialised_over_fused": round(med(t_m) / med(t_f), 3),
             "faster": "fused" if med(t_f) < med(t_m) else "materialised",
             "fused_output_frames_per_s": round((n + 1) / (med(t_f) * 1e-3)),
             "bytes_written": {"fused": out_bytes, "materialised": out_bytes + n * px * 16},
             "interior_pixels_with_full_reach": round(float(((nb == radius) & (nf == radius)).float().mean()), 4),
             "routes_bit_equal": bool(torch.equal(out[0], out[1]) and torch.equal(sup[0], sup[1])),
             "rounds_ms": {"fused": [round(x, 4) for x in t_f], "materialised": [round(x, 4) for x in t_m],
                           "materialised_filter_kernel": [round(x, 4) for x in t_s]}}
        if radius == 1:
            t_3 = times[3]
            r["batch_temporal_filter_ms"] = round(med(t_3), 4)
            r["fused_over_batch_temporal_filter"] = round(med(t_f) / med(t_3), 3)
            r["out_equals_batch_temporal_filter"] = bool(torch.equal(out[0], out[2]))
            r["rounds_ms"]["batch_temporal_filter"] = [round(x, 4) for x in t_3]
        print(json.dumps(r), flush=True)
        rows.append(r)
    sw, sh = p.level_size(p.sc_l)
    b.close()
    del out, sup, fw, rv
    torch.cuda.empty_cache()
    return rows, sw * sh * 8


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("trajfilter_probe.py measures on a GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    capi.check(capi.lib().ofdis_set_device(0))
    gray = clip(args.pairs + 1, dev)
    rgb = torch.stack([gray, 255 - gray, gray // 2 + 64], -1).contiguous()
    tstream = torch.cuda.Stream(device=dev)
    old = capi.set_tuning(contract=1)
    try:
        rows = []
        for frames, noc in ((gray, 1), (rgb, 3)):
            r, level_bytes = measure(frames, noc, tstream, dev, args.rounds, args.steps)
            rows += r
    finally:
        capi.restore_tuning(old)
    doc = {"tool": "tools/trajfilter_probe.py", "build_id": capi.build_id(), "device": torch.cuda.get_device_name(0),
           "geometry": f"{W}x{H} gray and RGB, operating point 2, TV on, fused contract for the flow, SEQUENCE | REVERSE "
                       f"context, one texture in periodic motion of at most ~1.2 px per pair; radius {list(RADII)}, flat weights "
                       f"1, tau = {TAU}, fb_check = 1, support written",
           "basis": "HIP events on one stream, warm-up, the routes timed alternately per round, median round; fused = "
                    "ofdis_batch_trajectory_filter; materialised = ofdis_batch_upsample_bidir (both flows, no masks: 16 bytes "
                    "per pixel and pair) + ofdis_trajectory_filter; bytes_written = out + support (+ those arrays); radius 1 "
                    "also against ofdis_batch_temporal_filter (wn = 1), reported only",
           "level_flow_bytes_per_pair_and_direction": level_bytes,
           "all_routes_bit_equal": all(r["routes_bit_equal"] for r in rows),
           "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "rows"}))


if __name__ == "__main__":
    main()
