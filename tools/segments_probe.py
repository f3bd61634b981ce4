"""Segments of label maps: ofdis_label_segments (conn 8, segments and records written) timed next to ofdis_motion_compensate,
the stage that feeds it, in the same job, on three inputs of 1024 maps of 1024x436:
  (a) the labels and residuals the affine and the projective compensate calls give on the clip of tools/track_probe.py (one
      texture in slow periodic motion), codes = OFDIS_GM_OUTLIER;
  (b) the same clip with a textured rectangle of RECT_W x RECT_H pasted in that moves on a circle of its own: affine labels,
      min_area RECT_MIN_AREA, and the IoU of the largest kept segment of every pair with the true rectangle in the pair's
      first frame;
  (c) random maps, every pixel foreground with probability 0.5, no flow.
Gray, operating point 2, TV on, fused contract for the flow passes (the kernels measured are independent of the contract), an
OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE context; full-resolution flow and mask from ofdis_batch_upsample_bidir, models from
3 rounds at thresh 1 with the mask.  HIP events on one non-default stream, warm-up first, the calls timed alternately in
several rounds; the median round is reported.  Bytes per pixel BY DESIGN (counted from of_dis_amd/csrc/ofdis_segments.hip, see
DESIGN.md "Segments": what every pixel moves whatever the map holds; the per-run and per-root accesses and the atomics come on
top) against bench.HBM_PEAK_GBS.

    python tools/segments_probe.py [--pairs 1024] [--out profiles/segments_probe.json]"""
import argparse
import json
import math
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
MAX_SEGMENTS = 256
RECT_W, RECT_H, RECT_MIN_AREA = 160, 96, 2000
# init 1 + 4, merge 1 (the row above hits in cache), flatten 1, count 4, number 4, relabel 1 + 4; the residual of a recorded
# foreground pixel 8 more
BYTES_PER_PIXEL = 20


def rect_origin(k):
    """top-left corner of the rectangle in frame k: a circle of radius 40 px, 3.5 px per frame"""
    a = 2 * math.pi * k / 72
    return int(round(W / 2 - RECT_W / 2 + 40 * math.cos(a))), int(round(H / 2 - RECT_H / 2 + 40 * math.sin(a)))


def with_rectangle(frames, dev):
    tex = bench.synth_frames_range(0, 1, W, H, 4321, dev)[0][0]
    out = frames.clone()
    for k in range(frames.shape[0]):
        x, y = rect_origin(k)
        out[k, y:y + RECT_H, x:x + RECT_W] = tex[100:100 + RECT_H, 300:300 + RECT_W]
    return out


class Route:
    """a context over the clip, its full-resolution flow and mask, and the two compensate calls writing residual and label"""

    def __init__(self, frames, tstream, dev):
        L, s = capi.lib(), tstream.cuda_stream
        self.L, self.s, n = L, s, frames.shape[0] - 1
        self.n = n
        p = oppoint(2, W, H, noc=1, usetvref=1, verbosity=0)
        b = capi.Batch(p, n, reverse=True, sequence=True)
        b.build_pyramids_u8_seq(frames.data_ptr(), W, H, stream=s)
        b.run(s)
        b.join(s)
        self.fw = torch.empty((n, H, W, 2), dtype=torch.float32, device=dev)
        self.mask = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
        capi.check(L.ofdis_batch_upsample_bidir(b.h, 0, n, self.fw.data_ptr(), None, self.mask.data_ptr(), None, W, H, capi.FB_ALPHA,
                                                capi.FB_BETA, s))
        tstream.synchronize()
        if b.status() != 0:
            raise SystemExit("the pass failed (ofdis_batch_status)")
        b.close()
        self.residual = torch.empty_like(self.fw)
        self.label = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
        self.models = {}
        for nparam, fit, wbytes in ((6, "ofdis_global_motion", L.ofdis_global_motion_work_bytes),
                                    (8, "ofdis_projective_motion", L.ofdis_projective_motion_work_bytes)):
            m = torch.empty((n, nparam), dtype=torch.float64, device=dev)
            wb = wbytes(n, W, H)
            work = torch.empty(wb, dtype=torch.uint8, device=dev)
            args = (self.fw.data_ptr(), self.mask.data_ptr(), n, W, H) + ((capi.GM_AFFINE,) if nparam == 6 else ()) + \
                (ROUNDS, THRESH, m.data_ptr(), None, work.data_ptr(), wb, s)
            capi.check(getattr(L, fit)(*args))
            tstream.synchronize()
            self.models[nparam] = m

    def compensate(self, nparam):
        fn = self.L.ofdis_motion_compensate if nparam == 6 else self.L.ofdis_projective_compensate
        capi.check(fn(self.fw.data_ptr(), self.mask.data_ptr(), self.models[nparam].data_ptr(), self.n, W, H, THRESH,
                      self.residual.data_ptr(), self.label.data_ptr(), self.s))


class Segments:
    def __init__(self, n, tstream, dev):
        self.L, self.s, self.n = capi.lib(), tstream.cuda_stream, n
        self.segments = torch.empty((n, H, W), dtype=torch.int32, device=dev)
        self.records = torch.zeros((n, MAX_SEGMENTS, capi.SEG_RECORD_FIELDS), dtype=torch.int64, device=dev)
        self.info = torch.zeros((n, capi.SEG_INFO_FIELDS), dtype=torch.int64, device=dev)
        self.wb = self.L.ofdis_segments_work_bytes(n, W, H)
        self.work = torch.empty(self.wb, dtype=torch.uint8, device=dev)

    def run(self, label, flow, codes, min_area):
        capi.check(self.L.ofdis_label_segments(label.data_ptr(), flow.data_ptr() if flow is not None else None, self.n, W, H, codes, 8,
                                               min_area, MAX_SEGMENTS, self.segments.data_ptr(), self.records.data_ptr(),
                                               self.info.data_ptr(), self.work.data_ptr(), self.wb, self.s))

    def summary(self):
        i = self.info.double()
        return {"components_per_map": round(float(i[:, 0].mean()), 1), "kept_per_map": round(float(i[:, 1].mean()), 1),
                "foreground_share": round(float(i[:, 3].mean()) / (W * H), 4),
                "largest_area": int(self.records[:, :, 0].max()) if int(self.info[:, 2].max()) else 0}


def row(name, n, t_seg, t_comp, seg, extra=None):
    med = statistics.median
    ms = med(t_seg)
    gbs = n * W * H * BYTES_PER_PIXEL / (ms * 1e-3) / 1e9
    r = {"input": name, "maps": n, "label_segments_ms": round(ms, 4), "maps_per_s": round(n / (ms * 1e-3)),
         "bytes_per_pixel_by_design": BYTES_PER_PIXEL, "design_gb_per_s": round(gbs, 1),
         "frac_of_hbm_peak": round(gbs / bench.HBM_PEAK_GBS, 4), **seg.summary(),
         "rounds_ms": [round(x, 4) for x in t_seg]}
    if t_comp is not None:
        r["motion_compensate_ms"] = round(med(t_comp), 4)
        r["label_segments_over_compensate"] = round(ms / med(t_comp), 3)
    r.update(extra or {})
    print(json.dumps(r), flush=True)
    return r


def rectangle_iou(seg, n, dev):
    """per pair: the largest recorded segment against the rectangle where frame k has it"""
    ious = []
    for k in range(n):
        nrec = int(seg.info[k, 2])
        if nrec == 0:
            ious.append(0.0)
            continue
        best = int(seg.records[k, :nrec, 0].argmax()) + 1
        got = seg.segments[k] == best
        x, y = rect_origin(k)
        true = torch.zeros((H, W), dtype=torch.bool, device=dev)
        true[y:y + RECT_H, x:x + RECT_W] = True
        ious.append(float((got & true).sum()) / float((got | true).sum()))
    return ious


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--inputs", default="abc", help="which of the inputs (a), (b), (c) to run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segments_probe.py measures on a GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    capi.check(capi.lib().ofdis_set_device(0))
    n = args.pairs
    tstream = torch.cuda.Stream(device=dev)
    seg = Segments(n, tstream, dev)
    moving = capi.SEG_MOVING
    rows = []
    # Every input below is made by torch on ITS stream and read by the library on tstream, a non-blocking stream that does not
    # wait for it: the device is synchronised after each is made.  ofdis_label_segments reads a map in several launches and
    # relies on reading the same bytes in each.
    old = capi.set_tuning(contract=1)
    try:
        if set(args.inputs) & set("ab"):
            frames = clip(n + 1, dev)
            torch.cuda.synchronize()
        if "a" in args.inputs:
            route = Route(frames, tstream, dev)
            for nparam, name in ((6, "(a) affine labels"), (8, "(a) projective labels")):
                route.compensate(nparam)
                t_seg, t_comp = alternate(tstream, [lambda: seg.run(route.label, route.residual, moving, 0),
                                                    lambda: route.compensate(nparam)], args.rounds, args.steps, 1)
                tstream.synchronize()
                rows.append(row(name, n, t_seg, t_comp, seg))
            del route
            torch.cuda.empty_cache()
        if "b" in args.inputs:
            pasted = with_rectangle(frames, dev)
            torch.cuda.synchronize()
            route = Route(pasted, tstream, dev)
            route.compensate(6)
            t_seg, t_comp = alternate(tstream, [lambda: seg.run(route.label, route.residual, moving, RECT_MIN_AREA),
                                                lambda: route.compensate(6)], args.rounds, args.steps, 1)
            tstream.synchronize()
            ious = rectangle_iou(seg, n, dev)
            rows.append(row("(b) affine labels, moving rectangle", n, t_seg, t_comp, seg,
                            {"min_area": RECT_MIN_AREA, "rectangle": [RECT_W, RECT_H],
                             "iou_largest_segment_vs_rectangle": {"median": round(statistics.median(ious), 4),
                                                                  "mean": round(statistics.fmean(ious), 4),
                                                                  "min": round(min(ious), 4), "max": round(max(ious), 4)}}))
            del route
            torch.cuda.empty_cache()
    finally:
        capi.restore_tuning(old)
    if "c" in args.inputs:
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        random = (torch.rand((n, H, W), device=dev, generator=gen) < 0.5).to(torch.uint8)
        torch.cuda.synchronize()
        (t_seg,) = alternate(tstream, [lambda: seg.run(random, None, 1 << 1, 0)], args.rounds, args.steps, 1)
        tstream.synchronize()
        rows.append(row("(c) random maps, density 0.5", n, t_seg, None, seg))
    doc = {"tool": "tools/segments_probe.py", "build_id": capi.build_id(), "device": torch.cuda.get_device_name(0),
           "geometry": f"{n} maps of {W}x{H}; conn 8, max_segments {MAX_SEGMENTS}, segments and records written, the residual as "
                       "flow in (a) and (b); labels of ofdis_motion_compensate / ofdis_projective_compensate (3 rounds, thresh 1, "
                       "forward-backward mask) on a SEQUENCE | REVERSE context at operating point 2",
           "basis": "HIP events on one stream, warm-up, the calls timed alternately per round, median round; motion_compensate = "
                    "the compensate call writing residual and label from the materialised flow, mask and models; "
                    f"bytes_per_pixel_by_design = {BYTES_PER_PIXEL}: what the seven launches move per pixel whatever the map holds "
                    f"(per-run and per-root accesses, the residual of recorded pixels and the atomics on top), against "
                    f"{bench.HBM_PEAK_GBS} GB/s; work buffer {seg.wb} bytes",
           "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "rows"}))


if __name__ == "__main__":
    main()
