"""Trajectory-aligned descriptors of the dense tracks of a clip: what ofdis_track_descriptors costs behind the materialised
route (ofdis_batch_upsample_bidir for all pairs, ofdis_dense_tracks on its two flow arrays), and the bytes it writes.

1024x436, operating point 2, TV on, fused arithmetic contract for the flow passes (the descriptor kernel is independent of the
contract), one GPU, an OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE context of 1024 pairs on the clip of tools/track_probe.py (one
texture in slow periodic motion).  Tracks as tools/dense_tracks_probe.py makes them: stride 5, window 2, max_len 15, min_eig the
median over the cells of frame 0 of the smaller eigenvalue.  Descriptors: N 32, nxy 2, nt 3 (D = 396), min_flow 0.4, on the gray
clip and on an RGB clip made of it (the gray frame, and the same frame shifted by 3 columns and by 5 rows, as the three
channels: only HOG reads the frames).  ntracks is read back once, before the timing, to size the arrays: dense_tracks runs a
second time with max_tracks = ntracks, so that hist has no idle slots.  HIP events on one non-default stream, warm-up first, the
variants timed alternately in several rounds; the median round is reported.  The gray result is compared with the numpy model
on the first tracks.

    python tools/descriptors_probe.py [--pairs 1024] [--out profiles/descriptors_probe.json]"""
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
from dense_tracks_probe import MAX_LEN, STRIDE, WINDOW, median_eigenvalue  # noqa: E402
from of_dis_amd import capi, tracking  # noqa: E402
from of_dis_amd.params import oppoint  # noqa: E402

W, H = track_probe.W, track_probe.H
PATCH, NXY, NT, MIN_FLOW = 32, 2, 3, 0.4
CHECKED_TRACKS = 2000  # compared with the numpy model


def dense_tracks(frames, fw, rv, n, min_eig, max_tracks, work, work_bytes, s, dev):
    """ofdis_dense_tracks with room for max_tracks: (tracks, start, len, info) on the device"""
    lmax = min(MAX_LEN, n)
    tracks = torch.empty((lmax + 1, max_tracks, 2), dtype=torch.float32, device=dev)
    start = torch.empty((max_tracks,), dtype=torch.int32, device=dev)
    length = torch.empty((max_tracks,), dtype=torch.int32, device=dev)
    info = torch.empty((2,), dtype=torch.int64, device=dev)
    capi.check(capi.lib().ofdis_dense_tracks(frames.data_ptr(), fw.data_ptr(), rv.data_ptr(), n, W, H, 1, STRIDE, WINDOW, min_eig,
                                             MAX_LEN, capi.FB_ALPHA, capi.FB_BETA, max_tracks, tracks.data_ptr(), start.data_ptr(),
                                             length.data_ptr(), info.data_ptr(), work.data_ptr(), work_bytes, s))
    return tracks, start, length, info


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
    ntracks, dropped = (int(x) for x in first[3].cpu())
    del first
    tracks, start, length, info = dense_tracks(frames, fw, rv, n, min_eig, ntracks, work, work_bytes, s, dev)
    tstream.synchronize()
    assert [int(x) for x in info.cpu()][0] == ntracks
    D = capi.track_descriptor_dims(PATCH, NXY, NT)
    rgb = torch.stack([frames, frames.roll(3, dims=2), frames.roll(5, dims=1)], dim=-1).contiguous()
    hist = torch.empty((ntracks, D), dtype=torch.int32, device=dev)
    shape = torch.empty((ntracks, lmax, 2), dtype=torch.float32, device=dev)

    def call(fr, noc, with_shape):
        capi.track_descriptors_dev(fr.data_ptr(), fw.data_ptr(), n, W, H, noc, tracks.data_ptr(), start.data_ptr(), length.data_ptr(),
                                   info.data_ptr(), lmax, ntracks, PATCH, NXY, NT, MIN_FLOW, hist.data_ptr(),
                                   shape.data_ptr() if with_shape else None, s)

    variants = [lambda: call(frames, 1, True), lambda: call(rgb, 3, True), lambda: call(frames, 1, False)]
    t_gray, t_rgb, t_noshape = track_probe.alternate(tstream, variants, rounds, steps, 2)
    call(frames, 1, True)
    tstream.synchronize()
    ln = length.cpu().numpy()
    # the first tracks against the numpy model (the model's time grows with the windows)
    k = min(CHECKED_TRACKS, ntracks)
    st = start[:k].cpu().numpy()
    last = max(int((st + ln[:k] - 1).max()) if k else 0, lmax)  # the frames those tracks reach
    want = tracking.track_descriptors_ref(frames[:last + 1].cpu().numpy(), fw[:last].cpu().numpy(),
                                          tracks[:, :k].cpu().numpy(), st, ln[:k], PATCH, NXY, NT, MIN_FLOW)
    equal = bool(np.array_equal(hist[:k].cpu().numpy().view(np.uint32), want[0])
                 and np.array_equal(shape[:k].cpu().numpy().view(np.uint32), want[1].view(np.uint32)))
    windows = int((ln - 1).sum())
    med = statistics.median
    r = {"pairs": n, "stride": STRIDE, "window": WINDOW, "max_len": MAX_LEN, "min_eig": min_eig, "tracks": ntracks, "dropped": dropped,
         "patch": PATCH, "nxy": NXY, "nt": NT, "min_flow": MIN_FLOW, "dims": D, "windows": windows,
         "window_pixels": windows * PATCH * PATCH,
         "gray_ms": round(med(t_gray), 4), "rgb_ms": round(med(t_rgb), 4), "gray_without_shape_ms": round(med(t_noshape), 4),
         "gray_windows_per_s": round(windows / (med(t_gray) * 1e-3)), "rgb_windows_per_s": round(windows / (med(t_rgb) * 1e-3)),
         "bytes_written": {"hist": ntracks * D * 4, "shape": ntracks * lmax * 8},
         "bytes_requested_per_window_pixel": {"gray": 5 * 8 + 4, "rgb": 5 * 8 + 12},
         "gray_written_GBs": round((ntracks * D * 4 + ntracks * lmax * 8) / (med(t_gray) * 1e-3) / 1e9, 2),
         "first_tracks_equal_the_model": equal, "tracks_checked": k,
         "rounds_ms": {"gray": [round(x, 4) for x in t_gray], "rgb": [round(x, 4) for x in t_rgb],
                       "gray_without_shape": [round(x, 4) for x in t_noshape]}}
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
        raise SystemExit("descriptors_probe.py measures on a GPU: no HIP device visible")
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
    doc = {"tool": "tools/descriptors_probe.py", "build_id": capi.build_id(), "device": torch.cuda.get_device_name(0),
           "geometry": f"{W}x{H}, operating point 2, TV on, fused contract for the flow, SEQUENCE | REVERSE context, one texture in "
                       f"periodic motion of at most ~1.2 px per pair; tracks of ofdis_dense_tracks on the materialised flows",
           "basis": "HIP events on one stream, warm-up, the variants timed alternately per round, median round; one call of "
                    "ofdis_track_descriptors for all tracks of the clip (hist and shape; gray frames, RGB frames, gray without "
                    "shape); windows = the sum of len - 1 over the tracks; bytes_written = hist and shape of the slots below "
                    "ntracks; bytes_requested_per_window_pixel = five flow values and four grey values, mostly cache hits",
           "first_tracks_equal_the_model": row["first_tracks_equal_the_model"],
           "rows": [row]}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "rows"}))


if __name__ == "__main__":
    main()
