"""Stereo with both views: what an OFDIS_BATCH_STEREO_LR context costs against a plain stereo context, and the fused finish
(ofdis_batch_upsample_lr) against the forward-only upsample (ofdis_batch_upsample_frames) and against the materialised
composition (upsample, lr_check twice, disparity_fill twice).

1242x375 gray, operating point 2, TV on, pyramids from resident 8-bit frames, both arithmetic contracts, one GPU.  Per batch
size the plain and the LR context live side by side and are timed alternately (host clock around `steps` calls and one
ofdis_sync, warm-up first, five rounds: median and spread are reported).  The yardstick of the pass is TWICE the plain
context's time; its own spread over the rounds is the margin.  The finish covers min(n, 1024) frames.

Algorithmic bytes: ofdis_batch_upsample_lr writes 10 B per output pixel (two floats, two mask bytes) and reads both level
disparities once; ofdis_batch_upsample_frames writes 4 B per pixel and reads one.  Fractions are of 8 TB/s.

    python tools/stereo_lr_probe.py [--sizes 1024,4096] [--out profiles/stereo_lr_probe.json]"""
import argparse
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
from of_dis_amd import capi  # noqa: E402
from of_dis_amd.params import oppoint, padded_size  # noqa: E402

W, H = 1242, 375
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


def free_bytes():
    try:
        import torch
        return torch.cuda.mem_get_info()[0]
    except Exception:
        return None


def measure(n, contract, rounds, steps):
    L = capi.lib()
    old = capi.set_tuning(contract=contract)
    p = oppoint(2, W, H, noc=1, usetvref=1).copy(selectmode=2)
    p.width, p.height = padded_size(W, H, p.sc_f)
    pairs = [gen_synth.make_pair(W, H, 1234 + k, 1)[:2] for k in range(4)]
    left = np.stack([pairs[k % 4][1] for k in range(n)])
    right = np.stack([pairs[k % 4][0] for k in range(n)])
    da, db = capi.Dev(left), capi.Dev(right)
    f0 = free_bytes()
    plain = capi.Batch(p, n)
    plain.build_pyramids_u8(da.ptr, db.ptr, W, H)
    capi.check(L.ofdis_sync(None))
    f1 = free_bytes()
    lr = capi.Batch(p, n, stereo_lr=True)
    lr.build_pyramids_u8(da.ptr, db.ptr, W, H)
    capi.check(L.ofdis_sync(None))
    f2 = free_bytes()
    if n >= 1024:  # as bench.py pipelines
        plain.set_pipeline(2)
        lr.set_pipeline(2)
    t_plain, t_lr = alternate([lambda: plain.run(), lambda: lr.run()], rounds, steps, 2)
    m = min(n, 1024)
    px = m * W * H
    out = [capi.Dev(nbytes=4 * px) for _ in range(4)]
    masks = [capi.Dev(nbytes=px) for _ in range(2)]

    def up_frames():
        capi.check(L.ofdis_batch_upsample_frames(plain.h, 0, m, out[0].ptr, W, H, None))

    def up_lr(fill):
        return lambda: capi.check(L.ofdis_batch_upsample_lr(lr.h, 0, m, out[0].ptr, out[1].ptr, masks[0].ptr, masks[1].ptr, fill,
                                                            W, H, 0.01, 0.5, None))

    def composition():  # U and Dm by the plain upsample (the un-mirroring is left out: it only flatters this route)
        capi.check(L.ofdis_batch_upsample_frames(plain.h, 0, m, out[2].ptr, W, H, None))
        capi.check(L.ofdis_batch_upsample_frames(lr.h, 0, m, out[3].ptr, W, H, None))
        capi.check(L.ofdis_lr_check(out[2].ptr, out[3].ptr, masks[0].ptr, m, W, H, 0.01, 0.5, None))
        capi.check(L.ofdis_lr_check(out[3].ptr, out[2].ptr, masks[1].ptr, m, W, H, 0.01, 0.5, None))
        capi.check(L.ofdis_disparity_fill(out[2].ptr, masks[0].ptr, out[0].ptr, m, W, H, capi.FILL_BACKGROUND, None))
        capi.check(L.ofdis_disparity_fill(out[3].ptr, masks[1].ptr, out[1].ptr, m, W, H, capi.FILL_BACKGROUND, None))

    t_up, t_none, t_bg, t_comp = alternate([up_frames, up_lr(capi.FILL_NONE), up_lr(capi.FILL_BACKGROUND), composition], rounds,
                                           steps, 2)
    lw, lh = p.level_size(p.sc_l)
    frac = lambda t, wr, levels: (px * wr + m * lw * lh * 4 * levels) / (t["median_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS
    res = {"pairs": n, "contract": "fused" if contract else "exact", "geometry": [W, H], "build_id": capi.build_id(),
           "pass_ms": {"plain": t_plain, "lr": t_lr, "lr_over_twice_plain": t_lr["median_ms"] / (2 * t_plain["median_ms"]),
                       "plain_spread": (t_plain["max_ms"] - t_plain["min_ms"]) / t_plain["median_ms"]},
           "finish_frames": m,
           "finish_ms": {"upsample_frames": t_up, "upsample_lr_fill_none": t_none, "upsample_lr_fill_background": t_bg,
                         "composition_background": t_comp},
           "hbm_frac_algorithmic": {"upsample_frames": frac(t_up, 4, 1), "upsample_lr_fill_none": frac(t_none, 10, 2),
                                    "upsample_lr_fill_background": frac(t_bg, 10, 2)},
           "context_bytes_per_pair": None if f0 is None else {"plain": (f0 - f1) / n, "lr": (f1 - f2) / n}}
    plain.close()
    lr.close()
    capi.restore_tuning(old)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    capi.check(capi.lib().ofdis_set_device(0))
    results = [measure(int(n), c, a.rounds, a.steps) for n in a.sizes.split(",") for c in (0, 1)]
    for r in results:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
