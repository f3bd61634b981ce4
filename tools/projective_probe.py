"""The 8-parameter projective camera models of a sequence context next to the affine ones, in one job on one context:
ofdis_batch_projective_motion + ofdis_batch_projective_compensate (fused: flows and codes straight from the level flows) against
the materialised route (ofdis_batch_upsample_bidir for all pairs, then ofdis_projective_motion and ofdis_projective_compensate on
its two arrays; its time includes that upsample), the same two routes of the affine twins, the bytes each route writes, and
for the standalone accumulate kernels (one round on the materialised arrays: flow and mask read once, 9 bytes per pixel) their
share of the HBM peak (bench.HBM_PEAK_GBS).

1024x436 gray, operating point 2, TV on, fused arithmetic contract for the flow passes (the fit kernels are independent of the
contract), one GPU, an OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE context of 1024 pairs over the clip of tools/track_probe.py.
3 rounds, thresh 1, fb_check = 1; compensate writes the labels only.  HIP events on one non-default stream, warm-up first, the
routes timed alternately in several rounds; the median round is reported.  Bit equality of the two routes is checked on the
models, the stats and the labels.

    python tools/projective_probe.py [--pairs 1024] [--out profiles/projective_probe.json]"""
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
from of_dis_amd import capi  # noqa: E402
from of_dis_amd.params import oppoint  # noqa: E402
from track_probe import H, W, alternate, clip  # noqa: E402

ROUNDS, THRESH = 3, 1.0


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
    fw = torch.empty((n, H, W, 2), dtype=torch.float32, device=dev)
    mf = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    a, be = capi.FB_ALPHA, capi.FB_BETA
    buf = {}
    for name, np_ in (("projective", 8), ("affine", 6)):
        wb = (L.ofdis_projective_motion_work_bytes if np_ == 8 else L.ofdis_global_motion_work_bytes)(n, W, H)
        buf[name] = dict(models=[torch.empty((n, np_), dtype=torch.float64, device=dev) for _ in range(2)],
                         stats=[torch.empty((n, 3), dtype=torch.int64, device=dev) for _ in range(2)],
                         label=[torch.empty((n, H, W), dtype=torch.uint8, device=dev) for _ in range(2)],
                         work=torch.empty(wb, dtype=torch.uint8, device=dev), work_bytes=wb)
    P, A = buf["projective"], buf["affine"]

    def upsample():
        capi.check(L.ofdis_batch_upsample_bidir(b.h, 0, n, fw.data_ptr(), None, mf.data_ptr(), None, W, H, a, be, s))

    def p_fused_fit():
        capi.check(L.ofdis_batch_projective_motion(b.h, 0, n, ROUNDS, THRESH, 1, a, be, P["models"][0].data_ptr(),
                                                   P["stats"][0].data_ptr(), W, H, s))

    def p_fused():
        p_fused_fit()
        capi.check(L.ofdis_batch_projective_compensate(b.h, 0, n, P["models"][0].data_ptr(), THRESH, 1, a, be, None,
                                                       P["label"][0].data_ptr(), W, H, s))

    def p_fit(rnds=ROUNDS):
        capi.check(L.ofdis_projective_motion(fw.data_ptr(), mf.data_ptr(), n, W, H, rnds, THRESH, P["models"][1].data_ptr(),
                                             P["stats"][1].data_ptr(), P["work"].data_ptr(), P["work_bytes"], s))

    def p_materialised():
        upsample()
        p_fit()
        capi.check(L.ofdis_projective_compensate(fw.data_ptr(), mf.data_ptr(), P["models"][1].data_ptr(), n, W, H, THRESH, None,
                                                 P["label"][1].data_ptr(), s))

    def a_fused_fit():
        capi.check(L.ofdis_batch_global_motion(b.h, 0, n, capi.GM_AFFINE, ROUNDS, THRESH, 1, a, be, A["models"][0].data_ptr(),
                                               A["stats"][0].data_ptr(), W, H, s))

    def a_fused():
        a_fused_fit()
        capi.check(L.ofdis_batch_motion_compensate(b.h, 0, n, A["models"][0].data_ptr(), THRESH, 1, a, be, None,
                                                   A["label"][0].data_ptr(), W, H, s))

    def a_fit(rnds=ROUNDS):
        capi.check(L.ofdis_global_motion(fw.data_ptr(), mf.data_ptr(), n, W, H, capi.GM_AFFINE, rnds, THRESH,
                                         A["models"][1].data_ptr(), A["stats"][1].data_ptr(), A["work"].data_ptr(),
                                         A["work_bytes"], s))

    def a_materialised():
        upsample()
        a_fit()
        capi.check(L.ofdis_motion_compensate(fw.data_ptr(), mf.data_ptr(), A["models"][1].data_ptr(), n, W, H, THRESH, None,
                                             A["label"][1].data_ptr(), s))

    fns = [p_fused, p_materialised, p_fused_fit, p_fit, a_fused, a_materialised, a_fused_fit, a_fit,
           lambda: p_fit(1), lambda: a_fit(1)]
    names = ["projective_fused", "projective_materialised", "projective_fused_fit_only", "projective_fit_kernels_only",
             "affine_fused", "affine_materialised", "affine_fused_fit_only", "affine_fit_kernels_only",
             "projective_one_round_standalone", "affine_one_round_standalone"]
    times = alternate(tstream, fns, rounds, steps, 2)
    # the models of the three-round fits once more (the one-round calls above wrote over them), then the comparison
    p_fused(), p_materialised(), a_fused(), a_materialised()
    tstream.synchronize()
    equal = {name: bool(torch.equal(d["models"][0].view(torch.int64), d["models"][1].view(torch.int64))
                        and torch.equal(d["stats"][0], d["stats"][1]) and torch.equal(d["label"][0], d["label"][1]))
             for name, d in buf.items()}
    med = {k: statistics.median(t) for k, t in zip(names, times)}
    px = W * H
    read_once = n * px * 9                     # the flow and the mask of every pixel
    frac = lambda ms: round(read_once / (ms * 1e-3) / (bench.HBM_PEAK_GBS * 1e9), 4)
    r = {"pairs": n, "rounds": ROUNDS, "thresh": THRESH,
         "ms": {k: round(v, 4) for k, v in med.items()},
         "projective_over_affine": {"fused_fit_only": round(med["projective_fused_fit_only"] / med["affine_fused_fit_only"], 3),
                                    "fit_kernels_only": round(med["projective_fit_kernels_only"] / med["affine_fit_kernels_only"], 3),
                                    "fused": round(med["projective_fused"] / med["affine_fused"], 3),
                                    "one_round_standalone": round(med["projective_one_round_standalone"]
                                                                  / med["affine_one_round_standalone"], 3)},
         "materialised_over_fused": {"projective": round(med["projective_materialised"] / med["projective_fused"], 3),
                                     "affine": round(med["affine_materialised"] / med["affine_fused"], 3)},
         "projective_fused_pairs_per_s": round(n / (med["projective_fused"] * 1e-3)),
         "bytes_written": {name: {"fused": n * (np_ * 8 + 24) + n * px + ROUNDS * buf[name]["work_bytes"],
                                  "materialised": n * (np_ * 8 + 24) + n * px + ROUNDS * buf[name]["work_bytes"] + n * px * 9}
                           for name, np_ in (("projective", 8), ("affine", 6))},
         "slab_bytes": {name: buf[name]["work_bytes"] for name in buf},
         "context_scratch_bytes": b.device_bytes() - before,
         # one standalone round = one accumulate launch that reads flow and mask once (+ the solve launch, one wavefront per pair)
         "accumulate_bytes_read": read_once,
         "accumulate_frac_of_hbm_peak": {"projective": frac(med["projective_one_round_standalone"]),
                                         "affine": frac(med["affine_one_round_standalone"])},
         "params_solved_counts": {str(k): int((P["stats"][0][:, 2] == k).sum()) for k in (8, 6, 2, 0)},
         "inlier_share_of_valid": {name: round(float((d["stats"][0][:, 1].double()
                                                      / d["stats"][0][:, 0].clamp(min=1).double()).mean()), 4)
                                   for name, d in buf.items()},
         "routes_bit_equal": equal,
         "rounds_ms": {k: [round(x, 4) for x in t] for k, t in zip(names, times)}}
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
        raise SystemExit("projective_probe.py measures on a GPU: no HIP device visible")
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
    doc = {"tool": "tools/projective_probe.py", "build_id": capi.build_id(), "device": torch.cuda.get_device_name(0),
           "geometry": f"{W}x{H} gray, operating point 2, TV on, fused contract for the flow, SEQUENCE | REVERSE context, one "
                       f"texture in periodic motion of at most ~1.2 px per pair; {ROUNDS} rounds, thresh {THRESH}, fb_check = 1, "
                       "labels written; the 8-parameter projective fit and the affine fit on the same context in one job",
           "basis": "HIP events on one stream, warm-up, the routes timed alternately per round, median round; fused = "
                    "ofdis_batch_*_motion + ofdis_batch_*_compensate; materialised = ofdis_batch_upsample_bidir (forward flow and "
                    "mask: 9 bytes per pixel and pair) + the standalone fit + compensate; bytes_written = models + stats + labels "
                    "+ the slab once per round (+ those arrays); accumulate_frac_of_hbm_peak = 9 bytes per pixel read once / the "
                    "time of a one-round standalone fit / bench.HBM_PEAK_GBS",
           "rows": [row]}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "rows"}))


if __name__ == "__main__":
    main()
