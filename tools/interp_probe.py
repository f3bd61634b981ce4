"""Frame interpolation from bidirectional flow: ofdis_batch_interpolate (fused: straight from a REVERSE context's level flows)
against the materialised route (ofdis_batch_upsample_bidir, then ofdis_interpolate on its four outputs), and the end-to-end
rate from resident 8-bit frames to interpolated frames.

1024x436 (the headline geometry), pyramids from resident 8-bit frames (bench.synth_frames_range): operating point 2 gray and
the RGB default operating point (2, noc 3), TV on, fused arithmetic contract for the flow passes (the interpolation itself is
independent of the contract), one GPU, 1024 and 4096 pairs, ntimes 1, 3 and 7 (times k / (ntimes + 1)).  HIP events on one
non-default stream, warm-up first, the two routes timed alternately in several rounds; the median round is reported.  The
materialised route runs in chunks of 1024 frames (its 18 B per output pixel of intermediates do not fit otherwise at 4096
pairs); its time is the sum over the chunks.

Compulsory bytes of one pair: both u8 frames read once, the ntimes output frames written once, both level flows read once.
Fractions are of 8 TB/s (bench.HBM_PEAK_GBS).  End to end = ofdis_batch_build_pyramids_u8 + ofdis_batch_run (REVERSE) +
ofdis_batch_interpolate, pipelined as bench.py pipelines.  Bit equality of the two routes is checked on frames 0..3 and the
last 4 of every batch.

    python tools/interp_probe.py [--sizes 1024,4096] [--times 1,3,7] [--out profiles/interp_probe.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from of_dis_amd import capi  # noqa: E402
from of_dis_amd.params import oppoint  # noqa: E402

W, H = 1024, 436
CHUNK = 1024


def timed(ts, fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ts)
    for _ in range(steps):
        fn()
    e1.record(ts)
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def alternate(ts, fns, rounds, steps, warmup):
    """median ms per call of each fn, the fns timed in turn within every round"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    res = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            res[k].append(timed(ts, fn, steps))
    return [statistics.median(r) for r in res], res


def measure(n, noc, ntimes_list, dev, rounds, steps):
    L = capi.lib()
    p = oppoint(2, W, H, noc=noc, usetvref=1, verbosity=0)
    ia, ib = bench.synth_frames_range(0, min(n, 64), W, H, 1234, dev, channels=noc)
    reps = (n + ia.shape[0] - 1) // ia.shape[0]
    rep = (reps,) + (1,) * (ia.dim() - 1)
    ia, ib = ia.repeat(*rep)[:n].contiguous(), ib.repeat(*rep)[:n].contiguous()
    tstream = torch.cuda.Stream(device=dev)
    s = tstream.cuda_stream
    b = capi.Batch(p, n, reverse=True)
    pipeline = 2 if n >= 1024 else 1
    b.set_pipeline(pipeline)
    torch.cuda.synchronize()
    b.build_pyramids_u8(ia.data_ptr(), ib.data_ptr(), W, H, s)
    b.run(s)
    b.join(s)
    torch.cuda.synchronize()
    sw, sh = p.level_size(p.sc_l)
    cnt = min(n, CHUNK)
    fw = torch.empty((cnt, H, W, 2), dtype=torch.float32, device=dev)
    rv = torch.empty_like(fw)
    mf = torch.empty((cnt, H, W), dtype=torch.uint8, device=dev)
    mr = torch.empty_like(mf)
    px = W * H * noc
    rows = []
    for nt in ntimes_list:
        times = np.array([(k + 1) / (nt + 1) for k in range(nt)], np.float32)
        tp = times.ctypes.data_as(capi.FP)
        out = torch.empty((n, nt, H, W) + ((noc,) if noc > 1 else ()), dtype=torch.uint8, device=dev)
        out_m = torch.empty((cnt, nt, H, W) + ((noc,) if noc > 1 else ()), dtype=torch.uint8, device=dev)

        def fused():
            capi.check(L.ofdis_batch_interpolate(b.h, ia.data_ptr(), ib.data_ptr(), 0, n, tp, nt, out.data_ptr(), W, H,
                                                 capi.FB_ALPHA, capi.FB_BETA, s))

        def materialised():
            for f0 in range(0, n, cnt):
                c = min(cnt, n - f0)
                capi.check(L.ofdis_batch_upsample_bidir(b.h, f0, c, fw.data_ptr(), rv.data_ptr(), mf.data_ptr(), mr.data_ptr(),
                                                        W, H, capi.FB_ALPHA, capi.FB_BETA, s))
                capi.check(L.ofdis_interpolate(ia[f0:].data_ptr(), ib[f0:].data_ptr(), fw.data_ptr(), rv.data_ptr(),
                                               mf.data_ptr(), mr.data_ptr(), out_m.data_ptr(), c, W, H, noc, tp, nt, s))
        (t_f, t_m), raw = alternate(tstream, [fused, materialised], rounds, steps, 2)
        # bit equality: frames 0..3 and the last 4, the materialised route run on those ranges alone
        equal = True
        for f0 in (0, max(0, n - 4)):
            c = min(4, n - f0)
            capi.check(L.ofdis_batch_upsample_bidir(b.h, f0, c, fw.data_ptr(), rv.data_ptr(), mf.data_ptr(), mr.data_ptr(), W, H,
                                                    capi.FB_ALPHA, capi.FB_BETA, s))
            capi.check(L.ofdis_interpolate(ia[f0:].data_ptr(), ib[f0:].data_ptr(), fw.data_ptr(), rv.data_ptr(), mf.data_ptr(),
                                           mr.data_ptr(), out_m.data_ptr(), c, W, H, noc, tp, nt, s))
            fused()
            tstream.synchronize()
            equal &= bool(torch.equal(out[f0:f0 + c], out_m[:c]))

        def e2e():
            b.build_pyramids_u8(ia.data_ptr(), ib.data_ptr(), W, H, s)
            b.run(s)
            fused()
        (t_e,), raw_e = alternate(tstream, [e2e], max(2, rounds // 2), 1, 1)
        comp = n * (2 * px + nt * px + 2 * sw * sh * 8)
        frac = lambda byt, ms: round(byt / (ms * 1e-3) / (bench.HBM_PEAK_GBS * 1e9), 4)
        r = {"pairs": n, "noc": noc, "op": 2, "ntimes": nt, "times": [float(t) for t in times], "pipeline": pipeline,
             "fused_ms": round(t_f, 4), "materialised_ms": round(t_m, 4),
             "fused_ms_per_1024_pairs": round(t_f * 1024 / n, 4), "materialised_over_fused": round(t_m / t_f, 3),
             "compulsory_bytes": comp, "fused_frac_of_8TBs": frac(comp, t_f), "materialised_frac_of_8TBs": frac(comp, t_m),
             "end_to_end_ms": round(t_e, 4), "end_to_end_pairs_per_s": round(n / (t_e * 1e-3)),
             "end_to_end_frames_per_s": round(n * nt / (t_e * 1e-3)),
             "routes_bit_equal": equal,
             "rounds_ms": {"fused": [round(x, 4) for x in raw[0]], "materialised": [round(x, 4) for x in raw[1]],
                           "end_to_end": [round(x, 4) for x in raw_e[0]]}}
        print(json.dumps(r), flush=True)
        rows.append(r)
        del out, out_m
    b.close()
    del fw, rv, mf, mr, ia, ib
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--times", default="1,3,7")
    ap.add_argument("--rgb-sizes", default=None, help="pair counts of the RGB rows (default: --sizes)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    capi.check(capi.lib().ofdis_set_device(0))
    old = capi.set_tuning(contract=1)
    nts = [int(x) for x in args.times.split(",")]
    rows = []
    try:
        for noc, sizes in ((1, args.sizes), (3, args.rgb_sizes or args.sizes)):
            for n in [int(x) for x in sizes.split(",")]:
                rows += measure(n, noc, nts, dev, args.rounds, args.steps)
    finally:
        capi.restore_tuning(old)
    doc = {"tool": "tools/interp_probe.py", "build_id": capi.build_id(), "device": torch.cuda.get_device_name(0),
           "geometry": f"{W}x{H}, operating point 2 gray and RGB, TV on, pyramids from 8-bit frames, fused contract for the flow",
           "basis": "HIP events, median of alternating rounds; compulsory bytes per pair: 2 u8 frames read + ntimes u8 frames "
                    "written + 2 level flows read; fractions of 8 TB/s; materialised = ofdis_batch_upsample_bidir + "
                    "ofdis_interpolate in chunks of 1024 frames",
           "all_routes_bit_equal": all(r["routes_bit_equal"] for r in rows),
           "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "rows"}))


if __name__ == "__main__":
    main()
