"""Compact output encodings: the fused call (ofdis_batch_upsample_frames_enc) against the fp32 upsample
(ofdis_batch_upsample_frames) and against the materialised composition (fp32 upsample, then ofdis_encode).

1024x436 gray, operating point 2, TV on, pyramids from resident 8-bit frames, one pass of the context, one GPU; then only the
finish is timed.  The routes are timed alternately (host clock around `steps` calls and one ofdis_sync, warm-up first, `rounds`
rounds: median, minimum and maximum are reported).  The fp32 upsample's own spread over the rounds is the margin the issue of
this tool sets for "not slower than the fp32 upsample".  --stereo measures the one-channel result of the stereo-depth mode.

Bytes: a route writes width x height x channels x element size per frame and reads the level flow once; the composition
additionally writes and re-reads the fp32 array.  `hbm_frac_written` is the bytes written divided by the time, as a share of
8 TB/s; `hbm_frac_algorithmic` adds the level flow's read.

    python tools/encode_probe.py [--pairs 4096] [--stereo] [--out profiles/encode_probe.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_synth  # noqa: E402
from of_dis_amd import capi, encoding  # noqa: E402
from of_dis_amd.params import oppoint, padded_size  # noqa: E402

W, H = 1024, 436
HBM_PEAK_GBS = 8000.0


def timed(fn, steps):
    L = capi.lib()
    capi.check(L.ofdis_sync(None))
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    capi.check(L.ofdis_sync(None))
    return (time.perf_counter() - t0) * 1e3 / steps


def alternate(fns, rounds, steps, warmup):
    for fn in fns:
        for _ in range(warmup):
            fn()
    res = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            res[k].append(timed(fn, steps))
    return [{"median_ms": statistics.median(r), "min_ms": min(r), "max_ms": max(r)} for r in res]


def measure(n, contract, stereo, rounds, steps):
    L = capi.lib()
    old = capi.set_tuning(contract=contract)
    p = oppoint(2, W, H, noc=1, usetvref=1)
    if stereo:
        p = p.copy(selectmode=2)
    p.width, p.height = padded_size(W, H, p.sc_f)
    pairs = [gen_synth.make_pair(W, H, 1234 + k, 1)[:2] for k in range(4)]
    da = capi.Dev(np.stack([pairs[k % 4][0] for k in range(n)]))
    db = capi.Dev(np.stack([pairs[k % 4][1] for k in range(n)]))
    b = capi.Batch(p, n)
    b.build_pyramids_u8(da.ptr, db.ptr, W, H)
    b.run()
    capi.check(L.ofdis_sync(None))
    vals = n * W * H * p.nop
    full = capi.Dev(nbytes=4 * vals)
    out = capi.Dev(nbytes=4 * vals)
    encs = {"f32": encoding.F32, "f16": encoding.F16,
            "u16": encoding.KITTI_DISPARITY if stereo else encoding.KITTI_FLOW, "u8": encoding.u8_bound(20)}

    def up_f32():  # (into the array the fused routes write: the routes compared differ in nothing but the call)
        capi.check(L.ofdis_batch_upsample_frames(b.h, 0, n, out.ptr, W, H, None))

    def fused(enc):
        return lambda: capi.check(L.ofdis_batch_upsample_frames_enc(b.h, 0, n, out.ptr, W, H, C.byref(enc), None))

    def composition(enc):
        def f():
            capi.check(L.ofdis_batch_upsample_frames(b.h, 0, n, full.ptr, W, H, None))
            capi.check(L.ofdis_encode(full.ptr, out.ptr, vals, C.byref(enc), None))
        return f

    names = list(encs)
    fns = [up_f32] + [fused(encs[k]) for k in names] + [composition(encs[k]) for k in names]
    t = alternate(fns, rounds, steps, 2)
    t_up, t_fused, t_comp = t[0], dict(zip(names, t[1:1 + len(names)])), dict(zip(names, t[1 + len(names):]))
    lw, lh = p.level_size(p.sc_l)
    level_bytes = n * lw * lh * p.nop * 4
    share = lambda tm, nbytes: nbytes / (tm["median_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS
    fracs = lambda tm, wr: {"hbm_frac_written": share(tm, wr), "hbm_frac_algorithmic": share(tm, wr + level_bytes)}
    spread = (t_up["max_ms"] - t_up["min_ms"]) / t_up["median_ms"]
    res = {"pairs": n, "contract": "fused" if contract else "exact", "mode": "stereo" if stereo else "flow", "geometry": [W, H],
           "build_id": capi.build_id(), "rounds": rounds, "steps": steps,
           "upsample_frames_f32": dict(t_up, spread=spread, **fracs(t_up, 4 * vals)), "encodings": {}}
    for k in names:
        wr = vals * encs[k].dtype.itemsize
        res["encodings"][k] = {
            "bytes_written": wr,
            "fused": dict(t_fused[k], **fracs(t_fused[k], wr)),
            "composition": t_comp[k],
            "fused_over_composition": t_fused[k]["median_ms"] / t_comp[k]["median_ms"],
            "fused_over_f32_upsample": t_fused[k]["median_ms"] / t_up["median_ms"],
            "faster_than_composition": t_fused[k]["median_ms"] < t_comp[k]["median_ms"],
            "not_slower_than_f32_upsample": t_fused[k]["median_ms"] <= t_up["median_ms"] * (1 + spread)}
    b.close()
    capi.restore_tuning(old)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--stereo", action="store_true")
    ap.add_argument("--contract", type=int, default=0, help="0 exact (the library default), 1 fused: the finish itself is the same code")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    capi.check(capi.lib().ofdis_set_device(0))
    results = [measure(a.pairs, a.contract, a.stereo, a.rounds, a.steps)]
    for r in results:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
