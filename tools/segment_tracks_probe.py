"""Object tracks: ofdis_segment_tracks (overlap, link, chain, relabel; track_map written) timed next to ofdis_label_segments,
the stage that feeds it, in the same job, on the clip (b) of tools/segments_probe.py: 1024 pairs of 1024x436, a textured
rectangle pasted in that moves 3.5 px per frame on a circle, affine labels, conn 8, min_area RECT_MIN_AREA.  Three values of
max_segments on the same maps: 128 (the overlap accumulated in LDS), 129 (the same maps through the global-atomics route: the
two routes side by side) and 256.  The four steps are timed one by one as well.  The flow is the context's full-resolution
forward flow (ofdis_batch_upsample_bidir); HIP events on one non-default stream, warm-up first, the calls timed alternately in
several rounds; the median round is reported.  Bytes per pixel BY DESIGN (counted from of_dis_amd/csrc/ofdis_segment_tracks.hip:
what every pixel moves whatever the maps hold): overlap reads 4 (segments), relabel reads 4 and writes 4 = 12 B; a recorded
pixel adds 8 B of flow and a gathered 4 B of the next map.  No threshold is set on any of this.

    python tools/segment_tracks_probe.py [--pairs 1024] [--out profiles/segment_tracks_probe.json]"""
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
from segments_probe import RECT_H, RECT_MIN_AREA, RECT_W, Route, with_rectangle  # noqa: E402
from track_probe import H, W, alternate, clip, timed  # noqa: E402

SEGMENT_SLOTS = (capi.SEGTRACK_LDS_MAX_SEGMENTS, capi.SEGTRACK_LDS_MAX_SEGMENTS + 1, 256)
MIN_SHARE = 50
BYTES_PER_PIXEL = 12


class Tracks:
    """the arrays of ofdis_label_segments and ofdis_segment_tracks for n maps and S segment slots"""

    def __init__(self, n, S, tstream, dev):
        self.L, self.s, self.n, self.S = capi.lib(), tstream.cuda_stream, n, S
        i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
        self.segments = torch.empty((n, H, W), **i32)
        self.records = torch.zeros((n, S, capi.SEG_RECORD_FIELDS), **i64)
        self.info = torch.zeros((n, capi.SEG_INFO_FIELDS), **i64)
        self.seg_wb = self.L.ofdis_segments_work_bytes(n, W, H)
        self.seg_work = torch.empty(self.seg_wb, dtype=torch.uint8, device=dev)
        self.max_tracks = min(n * S, capi.SEGTRACK_MAX_TRACKS)
        self.ids = torch.zeros((n, S), **i32)
        self.tracks = torch.zeros((self.max_tracks, capi.SEGTRACK_FIELDS), **i64)
        self.tinfo = torch.zeros(capi.SEGTRACK_INFO_FIELDS, **i64)
        self.track_map = torch.empty((n, H, W), **i32)
        self.wb = self.L.ofdis_segment_tracks_work_bytes(n, S)
        self.work = torch.empty(self.wb, dtype=torch.uint8, device=dev)
        self.overlap = self.work.data_ptr()
        self.link = self.overlap + (n - 1) * S * S * 4

    def label(self, label, flow):
        capi.check(self.L.ofdis_label_segments(label.data_ptr(), flow.data_ptr(), self.n, W, H, capi.SEG_MOVING, 8, RECT_MIN_AREA, self.S,
                                               self.segments.data_ptr(), self.records.data_ptr(), self.info.data_ptr(),
                                               self.seg_work.data_ptr(), self.seg_wb, self.s))

    def run(self, flow):
        capi.check(self.L.ofdis_segment_tracks(self.segments.data_ptr(), flow.data_ptr(), self.records.data_ptr(), self.info.data_ptr(),
                                               self.n, W, H, self.S, MIN_SHARE, self.max_tracks, self.ids.data_ptr(),
                                               self.tracks.data_ptr(), self.tinfo.data_ptr(), self.track_map.data_ptr(),
                                               self.work.data_ptr(), self.wb, self.s))

    def steps(self, flow):
        """the four calls, in order: name -> a function that enqueues it"""
        L, n, S, s = self.L, self.n, self.S, self.s
        seg, info, rec = self.segments.data_ptr(), self.info.data_ptr(), self.records.data_ptr()
        return {"overlap": lambda: capi.check(L.ofdis_segment_overlap(seg, flow.data_ptr(), info, n, W, H, S, self.overlap, s)),
                "link": lambda: capi.check(L.ofdis_segment_link(self.overlap, rec, info, n, S, MIN_SHARE, self.link, s)),
                "chain": lambda: capi.check(L.ofdis_segment_chain(self.link, rec, info, n, S, self.max_tracks, self.ids.data_ptr(),
                                                                  self.tracks.data_ptr(), self.tinfo.data_ptr(), s)),
                "relabel": lambda: capi.check(L.ofdis_segment_relabel(seg, self.ids.data_ptr(), info, n, W, H, S,
                                                                      self.track_map.data_ptr(), s))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segment_tracks_probe.py measures on a GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    capi.check(capi.lib().ofdis_set_device(0))
    n = args.pairs
    tstream = torch.cuda.Stream(device=dev)
    med = statistics.median
    old = capi.set_tuning(contract=1)
    try:
        # made by torch on ITS stream, read by the library on tstream, which does not wait for it: synchronise after each
        pasted = with_rectangle(clip(n + 1, dev), dev)
        torch.cuda.synchronize()
        route = Route(pasted, tstream, dev)
        route.compensate(6)
        tstream.synchronize()
    finally:
        capi.restore_tuning(old)
    rows = []
    for S in SEGMENT_SLOTS:
        t = Tracks(n, S, tstream, dev)
        t.label(route.label, route.residual)
        tstream.synchronize()
        t_tracks, t_label = alternate(tstream, [lambda: t.run(route.fw), lambda: t.label(route.label, route.residual)], args.rounds,
                                      args.steps, 1)
        steps = {}
        for name, fn in t.steps(route.fw).items():   # (in order: each leaves what the next one reads)
            fn()
            tstream.synchronize()
            steps[name + "_ms"] = round(med([timed(tstream, fn, args.steps) for _ in range(args.rounds)]), 4)
        tstream.synchronize()
        ms = med(t_tracks)
        gbs = n * W * H * BYTES_PER_PIXEL / (ms * 1e-3) / 1e9
        tinfo = t.tinfo.tolist()
        r = {"max_segments": S, "overlap_route": "lds" if S <= capi.SEGTRACK_LDS_MAX_SEGMENTS else "global", "maps": n,
             "segment_tracks_ms": round(ms, 4), "label_segments_ms": round(med(t_label), 4),
             "segment_tracks_over_label_segments": round(ms / med(t_label), 3), **steps,
             "bytes_per_pixel_by_design": BYTES_PER_PIXEL, "design_gb_per_s": round(gbs, 1),
             "frac_of_hbm_peak": round(gbs / bench.HBM_PEAK_GBS, 4), "recorded_per_map": round(float(t.info[:, 2].double().mean()), 2),
             "ntracks": tinfo[0], "links": tinfo[2], "longest_track": tinfo[3], "work_bytes": t.wb,
             "rounds_ms": [round(x, 4) for x in t_tracks]}
        print(json.dumps(r), flush=True)
        rows.append(r)
        del t
        torch.cuda.empty_cache()
    doc = {"tool": "tools/segment_tracks_probe.py", "build_id": capi.build_id(), "device": torch.cuda.get_device_name(0),
           "geometry": f"{n} maps of {W}x{H}: the clip of tools/track_probe.py with a {RECT_W}x{RECT_H} textured rectangle moving 3.5 px "
                       f"per frame on a circle; labels of ofdis_motion_compensate (3 rounds, thresh 1, forward-backward mask), "
                       f"ofdis_label_segments conn 8, min_area {RECT_MIN_AREA}; min_share {MIN_SHARE}, a track slot per segment slot, "
                       "track_map written; the flow is that of ofdis_batch_upsample_bidir",
           "basis": "HIP events on one stream, warm-up, ofdis_segment_tracks and ofdis_label_segments timed alternately per round, "
                    "median round; then the four steps one by one, median of as many rounds; bytes_per_pixel_by_design = "
                    f"{BYTES_PER_PIXEL} (segments read twice, track_map written; flow and the gathered next map only for recorded "
                    f"pixels) against {bench.HBM_PEAK_GBS} GB/s; no threshold is set",
           "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "rows"}))


if __name__ == "__main__":
    main()
