"""Segments of label maps: the definition of include/ofdis.h, section "Segments", in plain numpy / Python -- the model the
device call (capi.label_segments -> ofdis_label_segments) is compared with bit for bit.  Integers throughout; the one
floating-point step is the quantisation (int)rintf(u * 256.0f) of the global-motion section (gmotion.py).  Imports no scipy."""
import numpy as np

from .gmotion import GM_MAX_FLOW, GM_MAX_SIDE, GM_OUTLIER

# the limits the header states in prose (it adds no macro for them)
SEG_MAX_SEGMENTS = 1 << 24
SEG_RECORD_FIELDS = 12   # area, root, xmin, ymin, xmax, ymax, sx, sy, nflow, squ, sqv, 0
SEG_INFO_FIELDS = 4      # ncomp, nkept, min(nkept, max_segments), foreground pixels
SEG_MOVING = 1 << GM_OUTLIER   # codes of the moving objects of a compensate call's labels
SEG_BLOCK = 256          # pixels per block of counts in the work buffer

_f32 = np.float32


def segments_work_bytes(nmaps, w, h):
    """the formula ofdis_segments_work_bytes documents; 0 for the sizes it rejects"""
    if nmaps < 1 or w < 1 or h < 1 or w > GM_MAX_SIDE or h > GM_MAX_SIDE:
        return 0
    return nmaps * (8 * w * h + 16 * (-(-(w * h) // SEG_BLOCK)))


def foreground(label, codes):
    """label uint8 [...]: label < 8 and bit `label` of codes set"""
    label = np.asarray(label, np.uint8)
    lut = np.array([b < 8 and (codes >> b) & 1 for b in range(256)], bool)
    return lut[label]


def _roots(fg, conn):
    """fg bool [h, w] -> parent int64 [h * w]: for a foreground pixel the smallest raster index of its component, else -1.
    A sequential union-find in raster order: a pixel joins its left, upper and (conn 8) upper-left and upper-right neighbours,
    every union hangs the larger root below the smaller."""
    h, w = fg.shape
    parent = list(range(h * w))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r

    rows = fg.tolist()
    for y in range(h):
        row, above = rows[y], rows[y - 1] if y else None
        for x in range(w):
            if not row[x]:
                continue
            p = y * w + x
            near = []
            if x and row[x - 1]:
                near.append(p - 1)
            if above is not None:
                if above[x]:
                    near.append(p - w)
                if conn == 8:
                    if x and above[x - 1]:
                        near.append(p - w - 1)
                    if x + 1 < w and above[x + 1]:
                        near.append(p - w + 1)
            for q in near:
                a, b = find(p), find(q)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    out = np.full(h * w, -1, np.int64)
    for p in np.flatnonzero(fg.reshape(-1)).tolist():
        out[p] = find(p)
    return out


def label_segments_ref(label, flow=None, codes=SEG_MOVING, conn=8, min_area=0, max_segments=SEG_MAX_SEGMENTS, records_fill=None):
    """label uint8 [nmaps, h, w] (or [h, w]: one map), flow float32 [nmaps, h, w, 2] or None ->
    (segments int32 [nmaps, h, w], records int64 [nmaps, max_segments, 12], info int64 [nmaps, 4]).
    Only the record slots < info[:, 2] are defined; the others keep records_fill (an int64 array of that shape, or zeros)."""
    label = np.asarray(label, np.uint8)
    if label.ndim == 2:
        label = label[None]
        flow = None if flow is None else np.asarray(flow)[None]
    nmaps, h, w = label.shape
    if codes <= 0 or codes > 0xFF or conn not in (4, 8) or min_area < 0 or not 1 <= max_segments <= SEG_MAX_SEGMENTS:
        raise ValueError("label_segments_ref: arguments ofdis_label_segments rejects")
    if flow is not None:
        flow = np.asarray(flow, _f32).reshape(nmaps, h, w, 2)
    segments = np.zeros((nmaps, h, w), np.int32)
    records = np.zeros((nmaps, max_segments, SEG_RECORD_FIELDS), np.int64) if records_fill is None else \
        np.array(records_fill, np.int64).reshape(nmaps, max_segments, SEG_RECORD_FIELDS)
    info = np.zeros((nmaps, SEG_INFO_FIELDS), np.int64)
    ys, xs = np.divmod(np.arange(h * w, dtype=np.int64), w)
    for m in range(nmaps):
        fg = foreground(label[m], codes)
        root = _roots(fg, conn)
        on = root >= 0
        roots, inverse, area = np.unique(root[on], return_inverse=True, return_counts=True)   # ascending roots
        kept = area >= max(min_area, 1)
        number = np.where(kept, np.cumsum(kept), 0)
        seg = np.zeros(h * w, np.int64)
        seg[on] = number[inverse]
        segments[m] = seg.reshape(h, w)
        nkept = int(kept.sum())
        nrec = min(nkept, max_segments)
        info[m] = (len(roots), nkept, nrec, int(on.sum()))
        if flow is not None:
            with np.errstate(invalid="ignore", over="ignore"):
                u, v = flow[m, ..., 0].reshape(-1), flow[m, ..., 1].reshape(-1)
                usable = (np.abs(u) <= _f32(GM_MAX_FLOW)) & (np.abs(v) <= _f32(GM_MAX_FLOW))
                qu = np.where(usable, np.rint(np.where(usable, u, 0) * _f32(256.0)), 0).astype(np.int64)
                qv = np.where(usable, np.rint(np.where(usable, v, 0) * _f32(256.0)), 0).astype(np.int64)
        if nrec == 0:
            continue
        px = np.flatnonzero((seg >= 1) & (seg <= nrec))   # the pixels of the recorded segments, in raster order
        slot = seg[px] - 1
        rec = np.zeros((nrec, SEG_RECORD_FIELDS), np.int64)
        rec[:, (1, 2, 3)] = np.iinfo(np.int64).max
        for field, op, value in ((0, np.add, 1), (1, np.minimum, px), (2, np.minimum, xs[px]), (3, np.minimum, ys[px]),
                                 (4, np.maximum, xs[px]), (5, np.maximum, ys[px]), (6, np.add, xs[px]), (7, np.add, ys[px])):
            op.at(rec[:, field], slot, value)
        if flow is not None:
            for field, value in ((8, usable[px].astype(np.int64)), (9, qu[px]), (10, qv[px])):
                np.add.at(rec[:, field], slot, value)
        records[m, :nrec] = rec
    return segments, records, info
