"""Video sequence contexts (OFDIS_BATCH_SEQUENCE: n + 1 frames held once, pair k = frames k, k + 1) against plain contexts fed
every interior frame twice (img_a = frames[:-1], img_b = frames[1:]): the pyramid build alone, and the whole step from resident
8-bit frames to the u8 "bound 20" full-resolution flow (build + ofdis_batch_run + ofdis_batch_upsample_frames_enc), forward-only
and with OFDIS_BATCH_REVERSE, plus both contexts' ofdis_batch_device_bytes.

1024x436 gray, operating point 2, TV on, 4096 pairs, fused arithmetic contract, one GPU.  HIP events on one non-default stream,
warm-up first, the two variants of a configuration timed alternately in several rounds in the same process; the median round is
reported and every round is kept.  Both variants see the same pixels, so their encoded outputs are compared byte for byte.

What the byte counts predict for the build (to be compared with the measurement, not assumed): the base pass reads every frame
once instead of twice (0.5x) and the plane kernels write 3 (n + 1) planes instead of 6 n (reverse: 0.5x) or 4 n (forward-only:
0.75x, B has no gradient planes there).

    python tools/seqctx_probe.py [--pairs 4096] [--rounds 7] [--steps 3] [--out profiles/seqctx_probe.json]"""
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


def plane_bytes(p, n, planes_per_pair=None, planes_per_frame=None):
    elems = sum((p.level_size(l)[0] + 2 * p.imgpadding) * (p.level_size(l)[1] + 2 * p.imgpadding) * p.noc
                for l in range(p.sc_l, p.sc_f + 1))
    return 4 * elems * (planes_per_pair * n if planes_per_pair else planes_per_frame * (n + 1))


def measure(n, reverse, frames, dev, rounds, steps):
    L = capi.lib()
    p = oppoint(2, W, H, noc=1, usetvref=1, verbosity=0)
    tstream = torch.cuda.Stream(device=dev)
    s = tstream.cuda_stream
    plain = capi.Batch(p, n, reverse=reverse)
    seq = capi.Batch(p, n, reverse=reverse, sequence=True)
    pipeline = 2 if n >= 1024 else 1
    for b in (plain, seq):
        b.set_pipeline(pipeline)
    a_ptr, b_ptr = frames.data_ptr(), frames[1:].data_ptr()
    enc = capi.Encoding(capi.ENC_U8, 255.0 / 40.0, 127.5)
    outs = [torch.empty((n, H, W, 2), dtype=torch.uint8, device=dev) for _ in range(2)]

    def build_plain():
        plain.build_pyramids_u8(a_ptr, b_ptr, W, H, s)

    def build_seq():
        seq.build_pyramids_u8_seq(a_ptr, W, H, stream=s)

    def step(b, build, out):
        def fn():
            build()
            b.run(s)
            capi.check(L.ofdis_batch_upsample_frames_enc(b.h, 0, n, out.data_ptr(), W, H, capi.C.byref(enc), s))
        return fn
    step_plain, step_seq = step(plain, build_plain, outs[0]), step(seq, build_seq, outs[1])
    t_build = alternate(tstream, [build_plain, build_seq], rounds, steps, 2)
    t_step = alternate(tstream, [step_plain, step_seq], rounds, steps, 2)
    tstream.synchronize()
    equal = bool(torch.equal(outs[0], outs[1]))
    med = statistics.median
    r = {"pairs": n, "reverse": reverse, "pipeline": pipeline,
         "build_ms": {"plain": round(med(t_build[0]), 4), "sequence": round(med(t_build[1]), 4)},
         "build_sequence_over_plain": round(med(t_build[1]) / med(t_build[0]), 3),
         "step_ms": {"plain": round(med(t_step[0]), 4), "sequence": round(med(t_step[1]), 4)},
         "step_sequence_over_plain": round(med(t_step[1]) / med(t_step[0]), 3),
         "step_pairs_per_s": {"plain": round(n / (med(t_step[0]) * 1e-3)), "sequence": round(n / (med(t_step[1]) * 1e-3))},
         "device_bytes": {"plain": plain.device_bytes(), "sequence": seq.device_bytes()},
         "device_bytes_sequence_over_plain": round(seq.device_bytes() / plain.device_bytes(), 3),
         "build_bytes_expected": {  # u8 frames read + planes written (the unpadded level images in between not counted)
             "plain": 2 * n * W * H + plane_bytes(p, n, planes_per_pair=6 if reverse else 4),
             "sequence": (n + 1) * W * H + plane_bytes(p, n, planes_per_frame=3)},
         "encoded_outputs_equal": equal,
         "rounds_ms": {"build_plain": [round(x, 4) for x in t_build[0]], "build_sequence": [round(x, 4) for x in t_build[1]],
                       "step_plain": [round(x, 4) for x in t_step[0]], "step_sequence": [round(x, 4) for x in t_step[1]]}}
    print(json.dumps(r), flush=True)
    plain.close()
    seq.close()
    del outs
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seqctx_probe.py measures on a GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    capi.check(capi.lib().ofdis_set_device(0))
    n = args.pairs
    ia, ib = bench.synth_frames_range(0, min(n + 1, 64), W, H, 1234, dev, channels=1)
    clip = torch.stack([ia, ib], 1).reshape((-1,) + tuple(ia.shape[1:]))  # a0 b0 a1 b1 ...: no pair is (X, X)
    reps = (n + 1 + clip.shape[0] - 1) // clip.shape[0]
    frames = clip.repeat(reps, 1, 1)[:n + 1].contiguous()
    del ia, ib, clip
    old = capi.set_tuning(contract=1)
    try:
        rows = [measure(n, reverse, frames, dev, args.rounds, args.steps) for reverse in (False, True)]
    finally:
        capi.restore_tuning(old)
    doc = {"tool": "tools/seqctx_probe.py", "build_id": capi.build_id(), "device": torch.cuda.get_device_name(0),
           "geometry": f"{W}x{H} gray, operating point 2, TV on, fused contract, 8-bit frames resident, u8 bound-20 output",
           "basis": "HIP events on one stream, warm-up, plain and sequence timed alternately per round, median round; plain = "
                    "ofdis_batch_build_pyramids_u8(frames[:-1], frames[1:]); sequence = ofdis_batch_build_pyramids_u8_seq(frames)",
           "sequence_build_faster_in_both": all(r["build_sequence_over_plain"] < 1 for r in rows),
           "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "rows"}))


if __name__ == "__main__":
    main()
