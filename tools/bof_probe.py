"""Bag-of-features encoding of the dense-track descriptors of a clip: what the three calls ofdis_descriptor_normalize ->
ofdis_codebook_assign -> ofdis_bof_histogram cost, what the fused ofdis_track_bof costs, and the int8 rate of the assignment.

The workload of tools/descriptors_probe.py: 1024x436, operating point 2, TV on, fused arithmetic contract for the flow passes (the
encoding is integers and independent of the contract), one GPU, 1024 pairs, tracks of stride 5, window 2, max_len 15,
descriptors N 32, nxy 2, nt 3 (D = 396; channels of 96, 108, 96, 96 entries) on the gray clip.  The codebook: nwords = 4000 rows
drawn from the clip's own normalised descriptors (evenly spaced slots) -- a stand-in for a trained one (training:
tools/kmeans_probe.py); the work of the assignment does not depend on the words' values.  min_len = lmax + 1 (complete tracks).  HIP events
on one non-default stream, warm-up first, the two routes timed alternately in several rounds; the median round is reported.
Both routes must give the same bytes, and the first tracks are compared with the numpy model.

The int8 rate counts the multiply-adds of the definition, tracks x nwords x D x 2 operations, against the time of the route; the
matrix cores also multiply the padding of every channel to 128 entries (512 instead of 396), which is counted separately.  The
peak: v_mfma_i32_16x16x64_i8 issues every 16 cycles per SIMD, 2 x 16 x 16 x 64 operations, on 256 CUs x 4 SIMDs at 2.4 GHz =
5.03 Pop/s (twice the BF16 rate).

    python tools/bof_probe.py [--pairs 1024] [--out profiles/bof_probe.json]"""
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
from dense_tracks_probe import MAX_LEN, STRIDE, median_eigenvalue  # noqa: E402
from descriptors_probe import MIN_FLOW, NT, NXY, PATCH, H, W, dense_tracks  # noqa: E402
from of_dis_amd import capi, tracking  # noqa: E402
from of_dis_amd.params import oppoint  # noqa: E402

NWORDS = 4000
CHECKED_TRACKS = 256  # compared with the numpy model
PEAK_INT8_OPS = 256 * 4 * (2 * 16 * 16 * 64 / 16) * 2.4e9


def measure(b, n, frames, min_eig, tstream, dev, rounds, steps):
    L = capi.lib()
    s = tstream.cuda_stream
    lmax = min(MAX_LEN, n)
    fw = torch.empty((n, H, W, 2), dtype=torch.float32, device=dev)
    rv = torch.empty_like(fw)
    capi.check(L.ofdis_batch_upsample_bidir(b.h, 0, n, fw.data_ptr(), rv.data_ptr(), None, None, W, H, capi.FB_ALPHA, capi.FB_BETA, s))
    work_bytes = L.ofdis_dense_tracks_work_bytes(n, W, H, STRIDE)
    work = torch.empty((work_bytes,), dtype=torch.uint8, device=dev)
    ncx, ncy = tracking.dense_grid(W, H, STRIDE)
    first = dense_tracks(frames, fw, rv, n, min_eig, min(n * ncx * ncy, capi.DT_MAX_TRACKS), work, work_bytes, s, dev)
    tstream.synchronize()
    ntracks = int(first[3].cpu()[0])
    del first
    tracks, start, length, info = dense_tracks(frames, fw, rv, n, min_eig, ntracks, work, work_bytes, s, dev)
    D = capi.track_descriptor_dims(PATCH, NXY, NT)
    hist = torch.empty((ntracks, D), dtype=torch.int32, device=dev)
    capi.track_descriptors_dev(frames.data_ptr(), fw.data_ptr(), n, W, H, 1, tracks.data_ptr(), start.data_ptr(), length.data_ptr(),
                               info.data_ptr(), lmax, ntracks, PATCH, NXY, NT, MIN_FLOW, hist.data_ptr(), None, s)
    tstream.synchronize()
    del fw, rv, tracks, work

    desc = torch.empty((ntracks, D), dtype=torch.uint8, device=dev)
    words = [torch.empty((ntracks, 4), dtype=torch.int32, device=dev) for _ in range(2)]
    dist = torch.empty((ntracks, 4), dtype=torch.int32, device=dev)
    bof = [torch.empty((4, NWORDS), dtype=torch.int32, device=dev) for _ in range(2)]
    min_len = lmax + 1
    capi.check(L.ofdis_descriptor_normalize(hist.data_ptr(), info.data_ptr(), ntracks, NXY, NT, desc.data_ptr(), s))
    tstream.synchronize()
    codebook = desc[torch.linspace(0, ntracks - 1, NWORDS, device=dev).long()].contiguous()

    def normalize():
        capi.check(L.ofdis_descriptor_normalize(hist.data_ptr(), info.data_ptr(), ntracks, NXY, NT, desc.data_ptr(), s))

    def assign():
        capi.check(L.ofdis_codebook_assign(desc.data_ptr(), info.data_ptr(), ntracks, NXY, NT, codebook.data_ptr(), NWORDS,
                                           words[0].data_ptr(), dist.data_ptr(), s))

    def count():
        capi.check(L.ofdis_bof_histogram(words[0].data_ptr(), length.data_ptr(), info.data_ptr(), ntracks, NWORDS, min_len,
                                         bof[0].data_ptr(), s))

    def chain():
        normalize(), assign(), count()

    def fused():
        capi.track_bof_dev(hist.data_ptr(), length.data_ptr(), info.data_ptr(), ntracks, NXY, NT, codebook.data_ptr(), NWORDS, min_len,
                           bof[1].data_ptr(), words[1].data_ptr(), s)

    t_chain, t_fused, t_norm, t_assign, t_count = track_probe.alternate(tstream, [chain, fused, normalize, assign, count], rounds,
                                                                        steps, 2)
    chain(), fused()
    tstream.synchronize()
    same = bool(torch.equal(bof[0], bof[1]) and torch.equal(words[0], words[1]))
    k = min(CHECKED_TRACKS, ntracks)
    layout = tracking.descriptor_layout(PATCH, NXY, NT)
    want_desc = tracking.normalize_descriptors_u8(hist[:k].cpu().numpy().view(np.uint32), layout)
    want = tracking.codebook_assign_ref(want_desc, layout, codebook.cpu().numpy())
    equal = bool(np.array_equal(desc[:k].cpu().numpy(), want_desc) and np.array_equal(words[1][:k].cpu().numpy(), want[0])
                 and np.array_equal(dist[:k].cpu().numpy(), want[1]))
    counted = int((length >= min_len).sum())
    sums_ok = bool((bof[1].sum(1) == counted).all())
    med = statistics.median
    ops = ntracks * NWORDS * D * 2
    padded = ntracks * NWORDS * 512 * 2
    rate = lambda ms: ops / (ms * 1e-3)
    r = {"pairs": n, "tracks": ntracks, "counted_tracks": counted, "nxy": NXY, "nt": NT, "dims": D, "nwords": NWORDS, "min_len": min_len,
         "chain_ms": round(med(t_chain), 4), "fused_ms": round(med(t_fused), 4),
         "normalize_ms": round(med(t_norm), 4), "assign_ms": round(med(t_assign), 4), "histogram_ms": round(med(t_count), 4),
         "int8_ops": ops, "int8_ops_with_padding": padded,
         "assign_Tops": round(rate(med(t_assign)) / 1e12, 2), "fused_Tops": round(rate(med(t_fused)) / 1e12, 2),
         "assign_fraction_of_peak": round(rate(med(t_assign)) / PEAK_INT8_OPS, 4),
         "fused_fraction_of_peak": round(rate(med(t_fused)) / PEAK_INT8_OPS, 4),
         "assign_fraction_of_peak_with_padding": round(padded / (med(t_assign) * 1e-3) / PEAK_INT8_OPS, 4),
         "peak_int8_Tops": round(PEAK_INT8_OPS / 1e12, 1),
         "bytes": {"hist": ntracks * D * 4, "desc": ntracks * D, "codebook": NWORDS * D, "words": ntracks * 16, "bof": 16 * NWORDS},
         "routes_give_the_same_bytes": same, "rows_sum_to_the_counted_tracks": sums_ok,
         "first_tracks_equal_the_model": equal, "tracks_checked": k,
         "rounds_ms": {"chain": [round(x, 4) for x in t_chain], "fused": [round(x, 4) for x in t_fused],
                       "assign": [round(x, 4) for x in t_assign]}}
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
        raise SystemExit("bof_probe.py measures on a GPU: no HIP device visible")
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
    doc = {"tool": "tools/bof_probe.py", "build_id": capi.build_id(), "device": torch.cuda.get_device_name(0),
           "geometry": f"{W}x{H}, operating point 2, TV on, fused contract for the flow, SEQUENCE | REVERSE context, the clip and the "
                       f"tracks of tools/descriptors_probe.py; descriptors N {PATCH}, nxy {NXY}, nt {NT}; a codebook of {NWORDS} words "
                       f"drawn from the clip's own descriptors",
           "basis": "HIP events on one stream, warm-up, the routes timed alternately per round, median round; chain = "
                    "ofdis_descriptor_normalize + ofdis_codebook_assign (words and dist) + ofdis_bof_histogram, fused = ofdis_track_bof "
                    "(bof and words); int8_ops = tracks x nwords x D x 2, the multiply-adds of the definition; with padding: every "
                    "channel to 128 entries, what the matrix cores execute; the peak is 256 CUs x 4 SIMDs x 2048 operations per cycle "
                    "at 2.4 GHz",
           "routes_give_the_same_bytes": row["routes_give_the_same_bytes"],
           "first_tracks_equal_the_model": row["first_tracks_equal_the_model"],
           "rows": [row]}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "rows"}))


if __name__ == "__main__":
    main()
