"""Point trajectories through a sequence context: ofdis_batch_track_points (fused: straight from the level flows) against the
materialised route (ofdis_batch_upsample_bidir for all pairs, then ofdis_track_points on its two flow arrays; its time
includes that upsample), and the bytes each route writes.

1024x436 gray, operating point 2, TV on, fused arithmetic contract for the flow passes (the trajectory kernels are independent
of the contract), one GPU, an OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE context of 1024 pairs.  The clip is one texture in
slow periodic motion (the analytic flow of tools/gen_synth.py scaled by sin(2 pi k / 64): at most about 1.2 px per pair), so
that tracks live long and the kernels do the work a real clip gives them; the share of tracks that reach the last frame is
reported.  Seeds at frame 0: a stride-5 grid and every pixel.  HIP events on one non-default stream, warm-up first, the two
routes timed alternately in several rounds; the median round is reported.  Bit equality of the two routes is checked on the
whole track and count arrays.

    python tools/track_probe.py [--pairs 1024] [--out profiles/track_probe.json]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from of_dis_amd import capi, tracking  # noqa: E402
from of_dis_amd.params import oppoint  # noqa: E402

W, H = 1024, 436
PERIOD = 64


def timed(ts, fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ts)
    for _ in range(steps):
        fn()
    e1.record(ts)
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def alternate(ts, fns, rounds, steps, warmup):
    """ms per call of each fn in every round, the fns timed in turn within a round"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    res = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            res[k].append(timed(ts, fn, steps))
    return res


def clip(nframes, dev):
    """nframes u8 frames: the first synthetic frame of bench.py displaced by sin(2 pi k / PERIOD) times gen_synth's flow"""
    import torch.nn.functional as F
    tex = bench.synth_frames_range(0, 1, W, H, 1234, dev)[0][0].float()[None, None]
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                            indexing="ij")
    u = 6 + 4 * torch.sin(2 * math.pi * 0.7 * ys / H + 0.3) + 2 * torch.cos(2 * math.pi * 1.1 * xs / W)
    v = -3 + 3 * torch.cos(2 * math.pi * 0.9 * xs / W + 1)
    frames = []
    for k in range(min(nframes, PERIOD)):
        a = math.sin(2 * math.pi * k / PERIOD)
        grid = torch.stack([(xs - a * u) / (W - 1) * 2 - 1, (ys - a * v) / (H - 1) * 2 - 1], -1)[None]
        f = F.grid_sample(tex, grid, mode="bicubic", padding_mode="border", align_corners=True)
        frames.append(f.round().clamp(0, 255).to(torch.uint8)[0, 0])
    frames = torch.stack(frames)
    reps = (nframes + frames.shape[0] - 1) // frames.shape[0]
    return frames.repeat(reps, 1, 1)[:nframes].contiguous()


def measure(b, n, seeds_np, name, tstream, dev, rounds, steps):
    L = capi.lib()
    s = tstream.cuda_stream
    npoints = seeds_np.shape[0]
    seeds = torch.from_numpy(seeds_np).to(dev)
    tracks = [torch.empty((n + 1, npoints, 2), dtype=torch.float32, device=dev) for _ in range(2)]
    counts = [torch.empty((npoints,), dtype=torch.int32, device=dev) for _ in range(2)]
    fw = torch.empty((n, H, W, 2), dtype=torch.float32, device=dev)
    rv = torch.empty_like(fw)

    def fused():
        capi.check(L.ofdis_batch_track_points(b.h, 0, n, seeds.data_ptr(), None, npoints, 0, 1, capi.FB_ALPHA, capi.FB_BETA,
                                              tracks[0].data_ptr(), counts[0].data_ptr(), W, H, s))

    def upsample():
        capi.check(L.ofdis_batch_upsample_bidir(b.h, 0, n, fw.data_ptr(), rv.data_ptr(), None, None, W, H, capi.FB_ALPHA,
                                                capi.FB_BETA, s))

    def standalone():
        capi.check(L.ofdis_track_points(fw.data_ptr(), rv.data_ptr(), n, W, H, seeds.data_ptr(), None, npoints, 0, capi.FB_ALPHA,
                                        capi.FB_BETA, tracks[1].data_ptr(), counts[1].data_ptr(), s))

    def materialised():
        upsample()
        standalone()
    t_f, t_m, t_s = alternate(tstream, [fused, materialised, standalone], rounds, steps, 2)
    tstream.synchronize()
    equal = bool(torch.equal(tracks[0].view(torch.int32), tracks[1].view(torch.int32)) and torch.equal(counts[0], counts[1]))
    c = counts[0].cpu().numpy()
    med = statistics.median
    track_bytes = (n + 1) * npoints * 8 + npoints * 4
    flow_bytes = 2 * n * W * H * 8
    r = {"seeds": name, "points": npoints, "pairs": n,
         "fused_ms": round(med(t_f), 4), "materialised_ms": round(med(t_m), 4),
         "materialised_track_kernel_ms": round(med(t_s), 4),
         "materialised_over_fused": round(med(t_m) / med(t_f), 3),
         "faster": "fused" if med(t_f) < med(t_m) else "materialised",
         "fused_point_steps_per_s": round(float(c.sum()) / (med(t_f) * 1e-3)),
         "bytes_written": {"fused": track_bytes, "materialised": track_bytes + flow_bytes},
         "tracks_reaching_the_last_frame": round(float((c == n + 1).mean()), 4), "mean_count": round(float(c.mean()), 2),
         "routes_bit_equal": equal,
         "rounds_ms": {"fused": [round(x, 4) for x in t_f], "materialised": [round(x, 4) for x in t_m],
                       "materialised_track_kernel": [round(x, 4) for x in t_s]}}
    print(json.dumps(r), flush=True)
    del tracks, counts, fw, rv, seeds
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_probe.py measures on a GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    capi.check(capi.lib().ofdis_set_device(0))
    n = args.pairs
    frames = clip(n + 1, dev)
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
        rows = [measure(b, n, tracking.grid_seeds(W, H, 5), "stride-5 grid at frame 0", tstream, dev, args.rounds, args.steps),
                measure(b, n, tracking.grid_seeds(W, H, 1), "every pixel at frame 0", tstream, dev, args.rounds, args.steps)]
        sw, sh = p.level_size(p.sc_l)
        b.close()
    finally:
        capi.restore_tuning(old)
    doc = {"tool": "tools/track_probe.py", "build_id": capi.build_id(), "device": torch.cuda.get_device_name(0),
           "geometry": f"{W}x{H} gray, operating point 2, TV on, fused contract for the flow, SEQUENCE | REVERSE context, "
                       f"one texture in periodic motion of at most ~1.2 px per pair",
           "basis": "HIP events on one stream, warm-up, the routes timed alternately per round, median round; fused = "
                    "ofdis_batch_track_points; materialised = ofdis_batch_upsample_bidir (both flows, no masks) + "
                    "ofdis_track_points; bytes_written = tracks + counts (+ both full-resolution flow arrays)",
           "level_flow_bytes_per_pair_and_direction": sw * sh * 8,
           "all_routes_bit_equal": all(r["routes_bit_equal"] for r in rows),
           "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "rows"}))


if __name__ == "__main__":
    main()
