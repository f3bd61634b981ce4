"""Track selection on the dense tracks of a clip: which share of the tracks ofdis_track_select rejects and why, what the call
costs against the bytes it has to move, and what ofdis_track_descriptors + ofdis_track_bof cost on the selected set against the
full set.

The workload of tools/descriptors_probe.py and tools/bof_probe.py: 1024x436, operating point 2, TV on, fused arithmetic contract
for the flow passes (the selection is compiled once and independent of the contract), one GPU, an OFDIS_BATCH_SEQUENCE |
OFDIS_BATCH_REVERSE context of 1024 pairs, tracks of stride 5, window 2, max_len 15; affine camera models of
ofdis_batch_global_motion as tools/gmotion_probe.py fits them (3 rounds, thresh 1, forward mask); the default parameters of
ofdis_track_select_defaults; descriptors N 32, nxy 2, nt 3; a codebook of 4000 words drawn from the clip's own descriptors,
min_len = lmax + 1.  The selection runs twice, into two output sets: with the camera models, and without them (no track is
then taken out as camera motion); each set is described and encoded.

The comparison base is the full-set route, what the library did before the selection existed: ofdis_track_descriptors +
ofdis_track_bof on every track.  A selected route is the same two calls on a compacted set; ofdis_track_select is timed on
its own and added to it.  HIP events on one non-default stream, warm-up first, the routes timed alternately in several rounds;
the median round is reported.  The codes, the counts and the first kept tracks are compared with the numpy model, and the
histogram rows of the selected set with rows `index` of the full set.

The clip is SYNTHETIC (one texture in slow periodic motion): the shares per code, and with them the saving, are this clip's
and no property of real video.

The bytes of ofdis_track_select: classify reads start, len and the L positions of every slot (the second walk over the
positions is counted as cache hits) and writes code; scatter reads start, len and the lmax + 1 entries of the kept slots and
writes them, index and shape_out.  Against the HBM peak of 8 TB/s.

    python tools/track_select_probe.py [--pairs 1024] [--out profiles/track_select_probe.json]"""
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
from bof_probe import NWORDS  # noqa: E402
from dense_tracks_probe import MAX_LEN, STRIDE, median_eigenvalue  # noqa: E402
from descriptors_probe import MIN_FLOW, NT, NXY, PATCH, H, W, dense_tracks  # noqa: E402
from gmotion_probe import MODEL, ROUNDS, THRESH  # noqa: E402
from of_dis_amd import capi, tracking  # noqa: E402
from of_dis_amd.params import oppoint  # noqa: E402

CHECKED_TRACKS = 4096  # kept tracks compared with the numpy model entry by entry (the codes of all tracks are)
PEAK_HBM = 8.0e12


def measure(b, n, frames, min_eig, tstream, dev, rounds, steps):
    L = capi.lib()
    s = tstream.cuda_stream
    lmax = min(MAX_LEN, n)
    fw = torch.empty((n, H, W, 2), dtype=torch.float32, device=dev)
    rv = torch.empty_like(fw)
    capi.check(L.ofdis_batch_upsample_bidir(b.h, 0, n, fw.data_ptr(), rv.data_ptr(), None, None, W, H, capi.FB_ALPHA, capi.FB_BETA, s))
    models = torch.empty((n, 6), dtype=torch.float64, device=dev)
    capi.check(L.ofdis_batch_global_motion(b.h, 0, n, MODEL, ROUNDS, THRESH, 1, capi.FB_ALPHA, capi.FB_BETA, models.data_ptr(), None,
                                           W, H, s))
    work_bytes = L.ofdis_dense_tracks_work_bytes(n, W, H, STRIDE)
    work = torch.empty((work_bytes,), dtype=torch.uint8, device=dev)
    ncx, ncy = tracking.dense_grid(W, H, STRIDE)
    first = dense_tracks(frames, fw, rv, n, min_eig, min(n * ncx * ncy, capi.DT_MAX_TRACKS), work, work_bytes, s, dev)
    tstream.synchronize()
    ntracks = int(first[3].cpu()[0])
    del first
    tracks, start, length, info = dense_tracks(frames, fw, rv, n, min_eig, ntracks, work, work_bytes, s, dev)
    tstream.synchronize()
    del rv, work

    # the selection, with the camera models and without: two output sets with room for every track, so nothing is dropped
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    variants = ("with_models", "without_models")
    code = [torch.empty((ntracks,), dtype=torch.uint8, device=dev) for _ in variants]
    counts = [torch.empty((7,), dtype=torch.int64, device=dev) for _ in variants]
    sel = [(f32(lmax + 1, ntracks, 2), i32(ntracks), i32(ntracks), torch.empty((2,), dtype=torch.int64, device=dev)) for _ in variants]
    index = [i32(ntracks) for _ in variants]
    shape = [f32(ntracks, lmax, 2) for _ in variants]
    swork_bytes = capi.track_select_work_bytes(ntracks)
    swork = torch.empty((swork_bytes,), dtype=torch.uint8, device=dev)

    def select(v):
        capi.track_select_dev(tracks.data_ptr(), start.data_ptr(), length.data_ptr(), info.data_ptr(), lmax, ntracks, ntracks,
                              sel[v][0].data_ptr(), sel[v][1].data_ptr(), sel[v][2].data_ptr(), sel[v][3].data_ptr(), swork.data_ptr(),
                              swork_bytes, models.data_ptr() if v == 0 else None, n, W, H, None, code[v].data_ptr(),
                              counts[v].data_ptr(), index[v].data_ptr(), shape[v].data_ptr(), s)

    select(0), select(1)
    tstream.synchronize()
    per_code = [[int(x) for x in c.cpu()] for c in counts]
    nkept = [int(x[3].cpu()[0]) for x in sel]
    assert all(k == c[0] and sum(c) == ntracks for k, c in zip(nkept, per_code))

    # descriptors and the bag of features: on the full set (0) and on the two selected sets (1, 2)
    D = capi.track_descriptor_dims(PATCH, NXY, NT)
    sets = [(tracks, start, length, info)] + sel
    hist = [torch.empty((ntracks, D), dtype=torch.int32, device=dev) for _ in sets]

    def describe(k):
        t, st, ln, inf = sets[k]
        capi.track_descriptors_dev(frames.data_ptr(), fw.data_ptr(), n, W, H, 1, t.data_ptr(), st.data_ptr(), ln.data_ptr(), inf.data_ptr(),
                                   lmax, ntracks, PATCH, NXY, NT, MIN_FLOW, hist[k].data_ptr(), None, s)

    describe(0)
    desc = torch.empty((ntracks, D), dtype=torch.uint8, device=dev)
    capi.check(L.ofdis_descriptor_normalize(hist[0].data_ptr(), info.data_ptr(), ntracks, NXY, NT, desc.data_ptr(), s))
    tstream.synchronize()
    codebook = desc[torch.linspace(0, ntracks - 1, NWORDS, device=dev).long()].contiguous()
    del desc
    bof = [torch.empty((4, NWORDS), dtype=torch.int32, device=dev) for _ in sets]
    min_len = lmax + 1

    def encode(k):
        capi.track_bof_dev(hist[k].data_ptr(), sets[k][2].data_ptr(), sets[k][3].data_ptr(), ntracks, NXY, NT, codebook.data_ptr(), NWORDS,
                           min_len, bof[k].data_ptr(), None, s)

    fns = [lambda k=k: describe(k) for k in range(3)] + [lambda k=k: encode(k) for k in range(3)] + [lambda: select(0), lambda: select(1)]
    times = track_probe.alternate(tstream, fns, rounds, steps, 2)
    for fn in fns:
        fn()
    tstream.synchronize()
    med = statistics.median
    t_desc, t_bof, t_select = [med(t) for t in times[0:3]], [med(t) for t in times[3:6]], [med(t) for t in times[6:8]]

    # against the numpy model: every code, and the first kept tracks entry by entry; the rows of the selected sets
    tr, st, ln = tracks.cpu().numpy(), start.cpu().numpy(), length.cpu().numpy()
    L_sum = int(np.clip(ln, 0, lmax + 1).sum())
    full_ms = t_desc[0] + t_bof[0]
    r = {"pairs": n, "stride": STRIDE, "max_len": MAX_LEN, "tracks": ntracks,
         "descriptors_full_ms": round(t_desc[0], 4), "bof_full_ms": round(t_bof[0], 4), "full_route_ms": round(full_ms, 4)}
    for v, name in enumerate(variants):
        want = tracking.track_select_ref(tr, st, ln, models.cpu().numpy() if v == 0 else None, (W, H), max_out=CHECKED_TRACKS)
        k = int(want[5][0])
        equal = bool(np.array_equal(code[v].cpu().numpy(), want[0]) and per_code[v] == [int(x) for x in want[1]]
                     and np.array_equal(index[v][:k].cpu().numpy(), want[6])
                     and np.array_equal(sel[v][0][:, :k].cpu().numpy().view(np.uint32), want[2].view(np.uint32))
                     and np.array_equal(shape[v][:k].cpu().numpy().view(np.uint32), want[7].view(np.uint32)))
        rows_equal = bool(torch.equal(hist[v + 1][:nkept[v]], hist[0][index[v][:nkept[v]].long()]))
        moved = {"classify_read": ntracks * 8 + L_sum * 8, "classify_written": ntracks,
                 "scatter_read": nkept[v] * (8 + (lmax + 1) * 8), "scatter_written": nkept[v] * ((lmax + 1) * 8 + 12 + lmax * 8)}
        total = sum(moved.values())
        sel_ms = t_desc[v + 1] + t_bof[v + 1] + t_select[v]
        r[name] = {"kept": nkept[v], "share_per_code": {c: round(x / ntracks, 4) for c, x in zip(tracking.TS_NAMES, per_code[v])},
                   "tracks_per_code": dict(zip(tracking.TS_NAMES, per_code[v])),
                   "select_ms": round(t_select[v], 4), "select_bytes": moved, "select_bytes_total": total,
                   "select_GBs": round(total / (t_select[v] * 1e-3) / 1e9, 1),
                   "select_fraction_of_hbm_peak": round(total / (t_select[v] * 1e-3) / PEAK_HBM, 4),
                   "descriptors_selected_ms": round(t_desc[v + 1], 4), "bof_selected_ms": round(t_bof[v + 1], 4),
                   "selected_route_ms": round(sel_ms, 4), "selected_over_full": round(sel_ms / full_ms, 4),
                   "codes_and_first_kept_tracks_equal_the_model": equal, "kept_tracks_checked": k,
                   "selected_rows_equal_the_full_set_rows": rows_equal}
    names = ["descriptors_full", "descriptors_with_models", "descriptors_without_models", "bof_full", "bof_with_models",
             "bof_without_models", "select_with_models", "select_without_models"]
    r["rounds_ms"] = {name: [round(x, 4) for x in t] for name, t in zip(names, times)}
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
        raise SystemExit("track_select_probe.py measures on a GPU: no HIP device visible")
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
    doc = {"tool": "tools/track_select_probe.py", "build_id": capi.build_id(), "device": torch.cuda.get_device_name(0),
           "geometry": f"{W}x{H}, operating point 2, TV on, fused contract for the flow, SEQUENCE | REVERSE context, the clip and the "
                       f"tracks of tools/descriptors_probe.py; affine models of ofdis_batch_global_motion ({ROUNDS} rounds, thresh "
                       f"{THRESH}, forward mask); the default selection parameters; descriptors N {PATCH}, nxy {NXY}, nt {NT}; a "
                       f"codebook of {NWORDS} words drawn from the clip's own descriptors",
           "basis": "HIP events on one stream, warm-up, the routes timed alternately per round, median round; full route = "
                    "ofdis_track_descriptors + ofdis_track_bof on every track (the library before the selection existed), selected "
                    "route = ofdis_track_select + the same two calls on the compacted set; select_bytes = what the definition has to "
                    "move (the second walk over the positions counted as cache hits), against an HBM peak of 8 TB/s",
           "caveat": "the clip is synthetic: the share of tracks per code, and therefore the saving, is this clip's and no property of "
                     "real video",
           "codes_and_first_kept_tracks_equal_the_model": all(row[v]["codes_and_first_kept_tracks_equal_the_model"]
                                                              for v in ("with_models", "without_models")),
           "selected_rows_equal_the_full_set_rows": all(row[v]["selected_rows_equal_the_full_set_rows"]
                                                        for v in ("with_models", "without_models")),
           "rows": [row]}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "rows"}))


if __name__ == "__main__":
    main()
