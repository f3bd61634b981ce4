"""Bidirectional flow: what a REVERSE context (ofdis_batch_create_ex, OFDIS_BATCH_REVERSE) costs against a plain one, and the
one-launch full-resolution output of both directions with both masks (ofdis_batch_upsample_bidir) against the forward-only
upsample (ofdis_batch_upsample_frames) on the same frames.

1024x436 (the headline geometry), operating point 2, TV on, pyramids from resident 8-bit frames (bench.synth_frames_range),
both arithmetic contracts, one GPU.  Per batch size the plain and the REVERSE context live side by side and are timed
alternately (HIP events on one non-default stream, warm-up first, several rounds of several steps each; the median round is
reported).  A step is one ofdis_batch_run on resident pyramids, pipelined as bench.py pipelines (2 sub-batches from 1024
pairs on, else none).  The upsample comparison covers min(n, 1024) frames.

Compulsory bytes of ofdis_batch_upsample_bidir: 18 B per output pixel written (two 8-byte flows, two 1-byte masks) plus both
directions' level flows read once (8 B per level pixel each); of ofdis_batch_upsample_frames: 8 B per output pixel plus one
level flow.  Fractions are of 8 TB/s (bench.HBM_PEAK_GBS).

    python tools/bidir_probe.py [--sizes 16384,4096,64] [--out profiles/bidir_probe.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from of_dis_amd import capi  # noqa: E402
from of_dis_amd.params import oppoint  # noqa: E402

W, H = 1024, 436


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


def measure(n, contract, dev, rounds, steps):
    L = capi.lib()
    capi.set_tuning(contract=contract)
    p = oppoint(2, W, H, noc=1, usetvref=1, verbosity=0)
    ia, ib = bench.synth_frames_range(0, min(n, 64), W, H, 1234, dev)
    reps = (n + ia.shape[0] - 1) // ia.shape[0]
    ia, ib = ia.repeat(reps, 1, 1)[:n].contiguous(), ib.repeat(reps, 1, 1)[:n].contiguous()
    tstream = torch.cuda.Stream(device=dev)
    s = tstream.cuda_stream
    plain, rev = capi.Batch(p, n), capi.Batch(p, n, reverse=True)
    pipeline = 2 if n >= 1024 else 1
    for b in (plain, rev):
        b.set_pipeline(pipeline)
    torch.cuda.synchronize()
    for b in (plain, rev):
        b.build_pyramids_u8(ia.data_ptr(), ib.data_ptr(), W, H, s)
    del ia, ib

    def run(b):
        return lambda: b.run(s)
    (t_plain, t_rev), raw = alternate(tstream, [run(plain), run(rev)], rounds, steps, 2)
    for b in (plain, rev):
        b.join(s)
    torch.cuda.synchronize()
    cnt = min(n, 1024)
    sw, sh = p.level_size(p.sc_l)
    fw = torch.empty((cnt, H, W, 2), dtype=torch.float32, device=dev)
    rv = torch.empty_like(fw)
    mf = torch.empty((cnt, H, W), dtype=torch.uint8, device=dev)
    mr = torch.empty_like(mf)

    def up():
        capi.check(L.ofdis_batch_upsample_frames(plain.h, 0, cnt, fw.data_ptr(), W, H, s))

    def bidir():
        capi.check(L.ofdis_batch_upsample_bidir(rev.h, 0, cnt, fw.data_ptr(), rv.data_ptr(), mf.data_ptr(), mr.data_ptr(), W, H,
                                                capi.FB_ALPHA, capi.FB_BETA, s))
    (t_up, t_bi), raw_up = alternate(tstream, [up, bidir], rounds, max(3, steps), 2)
    consistent = float((mf == 0).float().mean().item())
    plain.close()
    rev.close()
    del fw, rv, mf, mr
    torch.cuda.empty_cache()
    b_bi = cnt * (W * H * 18 + 2 * sw * sh * 8)
    b_up = cnt * (W * H * 8 + sw * sh * 8)
    frac = lambda byt, ms: round(byt / (ms * 1e-3) / (bench.HBM_PEAK_GBS * 1e9), 4)
    return {
        "pairs": n, "contract": "fused" if contract else "exact", "pipeline": pipeline,
        "step_ms_plain": round(t_plain, 4), "step_ms_reverse": round(t_rev, 4), "reverse_over_plain": round(t_rev / t_plain, 4),
        "pairs_per_s_plain": round(n / (t_plain * 1e-3)), "pairs_per_s_reverse": round(n / (t_rev * 1e-3)),
        "step_rounds_ms": {"plain": [round(x, 4) for x in raw[0]], "reverse": [round(x, 4) for x in raw[1]]},
        "upsample_frames": cnt,
        "upsample_ms": round(t_up, 4), "upsample_bidir_ms": round(t_bi, 4), "bidir_over_upsample": round(t_bi / t_up, 4),
        "upsample_bytes": b_up, "upsample_bidir_bytes": b_bi,
        "upsample_frac_of_8TBs": frac(b_up, t_up), "upsample_bidir_frac_of_8TBs": frac(b_bi, t_bi),
        "upsample_bidir_frac_written_only": frac(cnt * W * H * 18, t_bi),
        "upsample_rounds_ms": {"upsample": [round(x, 4) for x in raw_up[0]], "bidir": [round(x, 4) for x in raw_up[1]]},
        "mask_fw_consistent_fraction": round(consistent, 4),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", default="16384,4096,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    capi.check(capi.lib().ofdis_set_device(0))
    old = capi.get_tuning()
    rows = []
    try:
        for contract in (1, 0):
            for n in [int(x) for x in args.sizes.split(",")]:
                r = measure(n, contract, dev, args.rounds, args.steps)
                rows.append(r)
                print(json.dumps(r), flush=True)
    finally:
        capi.restore_tuning(old)
    doc = {"tool": "tools/bidir_probe.py", "build_id": capi.build_id(), "device": torch.cuda.get_device_name(0),
           "geometry": f"{W}x{H} gray, operating point 2, TV on, pyramids from 8-bit frames",
           "basis": "step = one ofdis_batch_run on resident pyramids (HIP events, median of alternating rounds); upsample bytes: "
                    "bidir 18 B per output pixel written + 2 level flows read, forward-only 8 B per output pixel + 1 level flow "
                    "read; fractions of 8 TB/s",
           "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "rows"}))


if __name__ == "__main__":
    main()
