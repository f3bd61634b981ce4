"""K-means training of the bag-of-features codebook on the dense-track descriptors of a clip: what an iteration of
ofdis_codebook_train costs, split into its assignment (ofdis_codebook_assign) and its centre update (ofdis_codebook_update), the
update's bytes per second against the HBM peak, and what the training buys: the distortion per iteration.

The workload of tools/bof_probe.py: 1024x436, operating point 2, TV on, fused arithmetic contract for the flow passes (the
training is integers and independent of the contract), one GPU, 1024 pairs, tracks of stride 5, window 2, max_len 15, descriptors
N 32, nxy 2, nt 3 (D = 396) on the gray clip, nwords = 4000, min_len = lmax + 1 (complete tracks).  The codebook starts from
ofdis_codebook_seed -- the evenly drawn rows tools/bof_probe.py uses as its stand-in -- so iteration 0 of the run is that
codebook's distortion.  HIP events on one non-default stream, warm-up first, the calls timed alternately in several rounds; the
median round is reported.  The update's bytes: the member rows of desc read once, plus words (three times), rank, order and
the offsets written and read once each; the slab of partial sums is not counted.

Checked against the numpy model: the words of the first tracks against the trained codebook, and the rows of the first words of
one more update (their members taken from the device's words over all tracks).

    python tools/kmeans_probe.py [--pairs 1024] [--iters 10] [--out profiles/kmeans_probe.json]"""
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
from bof_probe import CHECKED_TRACKS, NWORDS  # noqa: E402
from dense_tracks_probe import MAX_LEN, STRIDE, median_eigenvalue  # noqa: E402
from descriptors_probe import MIN_FLOW, NT, NXY, PATCH, H, W, dense_tracks  # noqa: E402
from of_dis_amd import capi, tracking  # noqa: E402
from of_dis_amd.params import oppoint  # noqa: E402

HBM_PEAK_GBS = 8000.0
CHECKED_WORDS = 64  # rows of the update compared with the numpy model


def descriptors(b, n, frames, min_eig, tstream, dev):
    """the clip's tracks and their normalised descriptors: (desc u8 [ntracks][D], length, info, lmax)"""
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
    desc = torch.empty((ntracks, D), dtype=torch.uint8, device=dev)
    capi.check(L.ofdis_descriptor_normalize(hist.data_ptr(), info.data_ptr(), ntracks, NXY, NT, desc.data_ptr(), s))
    tstream.synchronize()
    return desc, length, info, lmax


def measure(desc, length, info, lmax, n, iters, tstream, dev, rounds, steps):
    L = capi.lib()
    s = tstream.cuda_stream
    ntracks, D = desc.shape
    min_len = lmax + 1
    codebook = torch.empty((NWORDS, D), dtype=torch.uint8, device=dev)
    words = torch.empty((ntracks, 4), dtype=torch.int32, device=dev)
    dist = torch.empty((ntracks, 4), dtype=torch.int32, device=dev)
    counts = torch.empty((4, NWORDS), dtype=torch.int32, device=dev)
    stats = torch.empty((iters, 4, 2), dtype=torch.int64, device=dev)
    work_bytes = capi.codebook_train_work_bytes(ntracks, NXY, NT, NWORDS)
    work = torch.empty((work_bytes,), dtype=torch.uint8, device=dev)
    a = (desc.data_ptr(), length.data_ptr(), info.data_ptr(), ntracks, NXY, NT, NWORDS, min_len)

    def seed():
        capi.check(L.ofdis_codebook_seed(*a, codebook.data_ptr(), s))

    def train():
        capi.codebook_train_dev(*a, iters, codebook.data_ptr(), words.data_ptr(), counts.data_ptr(), stats.data_ptr(), work.data_ptr(),
                                work_bytes, s)

    def assign():
        capi.check(L.ofdis_codebook_assign(desc.data_ptr(), info.data_ptr(), ntracks, NXY, NT, codebook.data_ptr(), NWORDS,
                                           words.data_ptr(), dist.data_ptr(), s))

    def update():
        capi.check(L.ofdis_codebook_update(desc.data_ptr(), words.data_ptr(), length.data_ptr(), info.data_ptr(), ntracks, NXY, NT,
                                           NWORDS, min_len, codebook.data_ptr(), counts.data_ptr(), work.data_ptr(), work_bytes, s))

    # the run that is reported: from the seed
    seed(), train()
    tstream.synchronize()
    st = stats.cpu().numpy()
    empty = int((counts == 0).sum())
    distortion = st[:, :, 1].sum(1)
    # the trained codebook against the model: the first tracks' words, and the first words' rows of one more update
    assign()
    tstream.synchronize()
    k = min(CHECKED_TRACKS, ntracks)
    layout = tracking.descriptor_layout(PATCH, NXY, NT)
    hdesc, hwords, hlen, hcb = desc.cpu().numpy(), words.cpu().numpy(), length.cpu().numpy(), codebook.cpu().numpy()
    want = tracking.codebook_assign_ref(hdesc[:k], layout, hcb)
    words_equal = bool(np.array_equal(hwords[:k], want[0]) and np.array_equal(dist[:k].cpu().numpy(), want[1]))
    update()
    tstream.synchronize()
    hnext, hcounts = codebook.cpu().numpy(), counts.cpu().numpy().view(np.uint32)
    member = hlen >= min_len
    rows_equal = True
    for c, seg in enumerate(tracking._channel_slices(layout)):
        for w in range(min(CHECKED_WORDS, NWORDS)):
            m = member & (hwords[:, c] == w)
            cnt = int(m.sum())
            row = (2 * hdesc[m][:, seg].astype(np.int64).sum(0) + cnt) // (2 * cnt) if cnt else hcb[w, seg]
            rows_equal &= bool(cnt == hcounts[c, w] and np.array_equal(hnext[w, seg], row))
    del hdesc

    t_train, t_assign, t_update, t_seed = track_probe.alternate(tstream, [train, assign, update, seed], rounds, steps, 1)
    med = statistics.median
    members = int(member.sum())
    upd_bytes = members * D + ntracks * 16 * 3 + ntracks * 16 * 2 + members * 4 * 4 * 2 + 2 * 16 * (NWORDS + 1) + 2 * 16 * NWORDS + NWORDS * D
    per_iter = med(t_train) / iters
    r = {"pairs": n, "tracks": ntracks, "members": members, "nxy": NXY, "nt": NT, "dims": D, "nwords": NWORDS, "min_len": min_len,
         "iters": iters, "train_ms": round(med(t_train), 4), "iteration_ms": round(per_iter, 4),
         "assign_ms": round(med(t_assign), 4), "update_ms": round(med(t_update), 4), "seed_ms": round(med(t_seed), 4),
         "update_share_of_an_iteration": round(med(t_update) / per_iter, 4),
         "update_bytes": upd_bytes, "update_GBs": round(upd_bytes / med(t_update) / 1e6, 1),
         "update_fraction_of_hbm_peak": round(upd_bytes / med(t_update) / 1e6 / HBM_PEAK_GBS, 4),
         "work_bytes": work_bytes,
         "distortion": [int(x) for x in distortion], "changed": [int(x) for x in st[:, :, 0].sum(1)],
         "final_over_seed_distortion": round(float(distortion[-1]) / float(max(distortion[0], 1)), 4),
         "distortion_is_monotone_per_channel": bool((np.diff(st[:, :, 1], axis=0) <= 0).all()),
         "empty_words_of_the_last_assignment": empty,
         "first_tracks_words_equal_the_model": words_equal, "tracks_checked": k,
         "first_words_rows_equal_the_model": rows_equal, "words_checked": min(CHECKED_WORDS, NWORDS),
         "rounds_ms": {"train": [round(x, 4) for x in t_train], "assign": [round(x, 4) for x in t_assign],
                       "update": [round(x, 4) for x in t_update]}}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_probe.py measures on a GPU: no HIP device visible")
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
        desc, length, info, lmax = descriptors(b, n, frames, min_eig, tstream, dev)
        b.close()
        row = measure(desc, length, info, lmax, n, args.iters, tstream, dev, args.rounds, args.steps)
    finally:
        capi.restore_tuning(old)
    doc = {"tool": "tools/kmeans_probe.py", "build_id": capi.build_id(), "device": torch.cuda.get_device_name(0),
           "geometry": f"{W}x{H}, operating point 2, TV on, fused contract for the flow, SEQUENCE | REVERSE context, the clip, the tracks "
                       f"and the descriptors of tools/bof_probe.py (N {PATCH}, nxy {NXY}, nt {NT}); {NWORDS} words from "
                       f"ofdis_codebook_seed, complete tracks, {args.iters} iterations",
           "basis": "HIP events on one stream, warm-up, the calls timed alternately per round, median round; train = "
                    "ofdis_codebook_train with stats (iters x (assignment + update)), assign = ofdis_codebook_assign (words and dist), "
                    "update = ofdis_codebook_update alone; update_bytes = the member rows of desc once, words three times, rank, order "
                    "and the offsets written and read, counts and the codebook written; distortion = the sum over the four channels "
                    "of stats[t][c][1], iteration 0 being the seed codebook's; the HBM peak is 8 TB/s",
           "first_tracks_words_equal_the_model": row["first_tracks_words_equal_the_model"],
           "first_words_rows_equal_the_model": row["first_words_rows_equal_the_model"],
           "rows": [row]}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "rows"}))


if __name__ == "__main__":
    main()
