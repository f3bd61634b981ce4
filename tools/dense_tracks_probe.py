"""Dense trajectories through a sequence context: ofdis_batch_dense_tracks (fused: straight from the level flows) against the
materialised route (ofdis_batch_upsample_bidir for all pairs, then ofdis_dense_tracks on its two flow arrays; its time includes
that upsample), and the bytes each route writes.

1024x436 gray, operating point 2, TV on, fused arithmetic contract for the flow passes (the trajectory kernels are independent
of the contract), one GPU, an OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE context of 1024 pairs on the clip of
tools/track_probe.py (one texture in slow periodic motion).  Stride 5, window 2, max_len 15; min_eig is the median over the
cells of frame 0 of the smaller eigenvalue (half of the cells seed there), taken from the numpy model.  A call is one texture
launch and three launches per frame, each depending on the one before: what the launches themselves cost is what this probe is
for.  HIP events on one non-default stream, warm-up first, the two routes timed alternately in several rounds; the median
round is reported.  Bit equality of the two routes is checked on info and on every slot below ntracks.

    python tools/dense_tracks_probe.py [--pairs 1024] [--out profiles/dense_tracks_probe.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import track_probe  # noqa: E402
from of_dis_amd import capi, tracking  # noqa: E402
from of_dis_amd.params import oppoint  # noqa: E402

W, H = track_probe.W, track_probe.H
STRIDE, WINDOW, MAX_LEN = 5, 2, 15


def median_eigenvalue(frame0):
    a, b, c = (x.astype(np.float64) for x in tracking.structure_tensor(frame0[None], STRIDE, WINDOW))
    return int(np.median(((a + c) - np.sqrt((a - c) ** 2 + 4 * b * b)) / 2))


def measure(b, n, frames, min_eig, tstream, dev, rounds, steps):
    L = capi.lib()
    s = tstream.cuda_stream
    ncx, ncy = tracking.dense_grid(W, H, STRIDE)
    max_tracks = min(n * ncx * ncy, capi.DT_MAX_TRACKS)
    lmax = min(MAX_LEN, n)
    tracks = [torch.empty((lmax + 1, max_tracks, 2), dtype=torch.float32, device=dev) for _ in range(2)]
    start = [torch.empty((max_tracks,), dtype=torch.int32, device=dev) for _ in range(2)]
    length = [torch.empty((max_tracks,), dtype=torch.int32, device=dev) for _ in range(2)]
    info = [torch.empty((2,), dtype=torch.int64, device=dev) for _ in range(2)]
    fw = torch.empty((n, H, W, 2), dtype=torch.float32, device=dev)
    rv = torch.empty_like(fw)
    work_bytes = L.ofdis_dense_tracks_work_bytes(n, W, H, STRIDE)
    work = torch.empty((work_bytes,), dtype=torch.uint8, device=dev)

    def fused():
        capi.check(L.ofdis_batch_dense_tracks(b.h, frames.data_ptr(), 0, n, STRIDE, WINDOW, min_eig, MAX_LEN, 1, capi.FB_ALPHA,
                                              capi.FB_BETA, max_tracks, tracks[0].data_ptr(), start[0].data_ptr(),
                                              length[0].data_ptr(), info[0].data_ptr(), W, H, s))

    def upsample():
        capi.check(L.ofdis_batch_upsample_bidir(b.h, 0, n, fw.data_ptr(), rv.data_ptr(), None, None, W, H, capi.FB_ALPHA,
                                                capi.FB_BETA, s))

    def standalone():
        capi.check(L.ofdis_dense_tracks(frames.data_ptr(), fw.data_ptr(), rv.data_ptr(), n, W, H, 1, STRIDE, WINDOW, min_eig,
                                        MAX_LEN, capi.FB_ALPHA, capi.FB_BETA, max_tracks, tracks[1].data_ptr(),
                                        start[1].data_ptr(), length[1].data_ptr(), info[1].data_ptr(), work.data_ptr(), work_bytes,
                                        s))

    def materialised():
        upsample()
        standalone()
    before = b.device_bytes()
    t_f, t_m, t_s = track_probe.alternate(tstream, [fused, materialised, standalone], rounds, steps, 2)
    tstream.synchronize()
    nt, dropped = (int(x) for x in info[0].cpu())
    equal = bool(torch.equal(info[0], info[1]) and torch.equal(start[0][:nt], start[1][:nt])
                 and torch.equal(length[0][:nt], length[1][:nt])
                 and torch.equal(tracks[0][:, :nt].view(torch.int32), tracks[1][:, :nt].view(torch.int32)))
    ln, st = length[0][:nt].cpu().numpy(), start[0][:nt].cpu().numpy()
    med = statistics.median
    track_bytes = (lmax + 1) * nt * 8 + nt * 8 + 16
    flow_bytes = 2 * n * W * H * 8
    r = {"pairs": n, "stride": STRIDE, "window": WINDOW, "max_len": MAX_LEN, "min_eig": min_eig, "cells": ncx * ncy,
         "launches_per_call": 1 + 3 * n, "tracks": nt, "dropped": dropped, "reseeds": int((st > 0).sum()),
         "complete": round(float((ln == lmax + 1).mean()), 4), "mean_len": round(float(ln.mean()), 2),
         "fused_ms": round(med(t_f), 4), "materialised_ms": round(med(t_m), 4),
         "materialised_dense_tracks_ms": round(med(t_s), 4),
         "materialised_over_fused": round(med(t_m) / med(t_f), 3),
         "fused_us_per_frame": round(med(t_f) * 1e3 / (n + 1), 2),
         "fused_track_steps_per_s": round(float((ln - 1).sum()) / (med(t_f) * 1e-3)),
         "bytes_written": {"fused": track_bytes, "materialised": track_bytes + flow_bytes},
         "work_bytes": {"context": b.device_bytes() - before, "standalone": work_bytes},
         "routes_bit_equal": equal,
         "rounds_ms": {"fused": [round(x, 4) for x in t_f], "materialised": [round(x, 4) for x in t_m],
                       "materialised_dense_tracks": [round(x, 4) for x in t_s]}}
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
        raise SystemExit("dense_tracks_probe.py measures on a GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    capi.check(capi.lib().ofdis_set_device(0))
    n = args.pairs
    frames = track_probe.clip(n + 1, dev)
    min_eig = median_eigenvalue(frames[0].cpu().numpy())
    p = oppoint(2, W, H, noc=1, usetvref=1, verbosity=0)
    tstream = torch.cuda.Stream(device=dev)
    old = capi.set_tuning(contract=1)
    try:
        b = capi.Batch(p, n, reverse=True, sequence=True)
        b.build_pyramids_u8_seq(frames.data_ptr(), W, H, stream=tstream.cuda_stream)
        b.run(tstream.cuda_stream)
        b.join(tstream.cuda_stream)
        tstream.synchronize()
        if b.status() != 0:
            raise SystemExit("the pass failed (ofdis_batch_status)")
        row = measure(b, n, frames, min_eig, tstream, dev, args.rounds, args.steps)
        b.close()
    finally:
        capi.restore_tuning(old)
    doc = {"tool": "tools/dense_tracks_probe.py", "build_id": capi.build_id(), "device": torch.cuda.get_device_name(0),
           "geometry": f"{W}x{H} gray, operating point 2, TV on, fused contract for the flow, SEQUENCE | REVERSE context, "
                       f"one texture in periodic motion of at most ~1.2 px per pair",
           "basis": "HIP events on one stream, warm-up, the routes timed alternately per round, median round; fused = "
                    "ofdis_batch_dense_tracks; materialised = ofdis_batch_upsample_bidir (both flows, no masks) + "
                    "ofdis_dense_tracks; bytes_written = the slots below ntracks of tracks, start and len, and info (+ both "
                    "full-resolution flow arrays)",
           "all_routes_bit_equal": row["routes_bit_equal"],
           "rows": [row]}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "rows"}))


if __name__ == "__main__":
    main()
