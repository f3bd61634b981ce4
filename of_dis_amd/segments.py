"""Segments of label maps: the definition of include/ofdis.h, section "Segments", in plain numpy / Python -- the model the
device call (capi.label_segments -> ofdis_label_segments) is compared with bit for bit.  Integers throughout; the one
floating-point step is the quantisation (int)rintf(u * 256.0f) of the global-motion section (gmotion.py).  Imports no scipy.
Below it the definitions of the section "Object tracks": the segments of a clip's maps linked across frames (segment_overlap_ref,
segment_link_ref, segment_chain_ref, segment_relabel_ref, segment_tracks_ref), the model of capi.segment_tracks and its steps."""
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


# ------------------------------------------------------------------ object tracks
# include/ofdis.h, section "Object tracks": the definitions the device calls (capi.segment_overlap, _link, _chain, _relabel,
# _tracks) are compared with bit for bit; the limits that section states in prose
SEGTRACK_MAX_SEGMENTS = 1024
SEGTRACK_MAX_MAPS = 65536
SEGTRACK_MAX_TRACKS = 1 << 24
SEGTRACK_FIELDS = 12     # first_map, first_segment, length, last_segment, sums of area, sx, sy, nflow, squ, sqv, min area, max area
SEGTRACK_INFO_FIELDS = 4   # ntracks, min(ntracks, max_tracks), links followed, longest length
SEGTRACK_LDS_MAX_SEGMENTS = 128   # up to here the overlap is accumulated in LDS (the same bits either way)
SEGTRACK_MAX_AREA = 1 << 26


def segment_tracks_work_bytes(nmaps, max_segments):
    """the formula ofdis_segment_tracks_work_bytes documents; 0 for the arguments it rejects"""
    if not 1 <= nmaps <= SEGTRACK_MAX_MAPS or not 1 <= max_segments <= SEGTRACK_MAX_SEGMENTS:
        return 0
    return max(8, 8 * (-(-((nmaps - 1) * max_segments * (max_segments + 1) * 4) // 8)))


def _track_args(nmaps, max_segments, min_share=0, max_tracks=1):
    if not (1 <= nmaps <= SEGTRACK_MAX_MAPS and 1 <= max_segments <= SEGTRACK_MAX_SEGMENTS and 0 <= min_share <= 100
            and 1 <= max_tracks <= SEGTRACK_MAX_TRACKS):
        raise ValueError("segment tracks: arguments the device calls reject")


def recorded_counts(info, max_segments):
    """n_k = min(max(info[k][2], 0), S) for every map"""
    return np.clip(np.asarray(info, np.int64).reshape(-1, SEG_INFO_FIELDS)[:, 2], 0, max_segments).astype(np.int64)


def _filled(fill, shape, dtype):
    return np.zeros(shape, dtype) if fill is None else np.array(fill, dtype).reshape(shape)


def segment_overlap_ref(segments, flow, info, max_segments, overlap_fill=None):
    """segments int32 [N, h, w], flow float32 [N, h, w, 2], info int64 [N, 4] -> overlap int32 [N - 1, S, S]: the entries
    [k, :n_k, :n_{k+1}] are defined, the others keep overlap_fill (or zeros)"""
    segments = np.asarray(segments, np.int32)
    N, h, w = segments.shape
    S = max_segments
    _track_args(N, S)
    flow = np.asarray(flow, _f32).reshape(N, h, w, 2)
    n = recorded_counts(info, S)
    overlap = _filled(overlap_fill, (N - 1, S, S), np.int32)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    for k in range(N - 1):
        a = segments[k].astype(np.int64)
        u, v = flow[k, ..., 0], flow[k, ..., 1]
        with np.errstate(invalid="ignore"):
            usable = (np.abs(u) <= _f32(GM_MAX_FLOW)) & (np.abs(v) <= _f32(GM_MAX_FLOW))   # (a NaN fails)
        xt = xs + np.rint(np.where(usable, u, 0)).astype(np.int64)   # (rint: to nearest even, as rintf)
        yt = ys + np.rint(np.where(usable, v, 0)).astype(np.int64)
        ok = (a >= 1) & (a <= n[k]) & usable & (xt >= 0) & (xt < w) & (yt >= 0) & (yt < h)
        a, b = a[ok], segments[k + 1][yt[ok], xt[ok]].astype(np.int64)
        hit = (b >= 1) & (b <= n[k + 1])
        count = np.zeros((n[k], n[k + 1]), np.int64)
        np.add.at(count, (a[hit] - 1, b[hit] - 1), 1)
        overlap[k, :n[k], :n[k + 1]] = count
    return overlap


def segment_areas(records, max_segments):
    """records[..., 0] clamped to 0 .. 2^26: [N, S]"""
    return np.clip(np.asarray(records, np.int64).reshape(-1, max_segments, SEG_RECORD_FIELDS)[:, :, 0], 0, SEGTRACK_MAX_AREA)


def segment_link_ref(overlap, records, info, max_segments, min_share, link_fill=None):
    """overlap int32 [N - 1, S, S], records int64 [N, S, 12], info int64 [N, 4] -> link int32 [N - 1, S]: the entries
    [k, :n_k] are defined (b, or 0), the others keep link_fill (or zeros)"""
    S = max_segments
    n = recorded_counts(info, S)
    N = len(n)
    _track_args(N, S, min_share)
    overlap = np.asarray(overlap, np.int32).reshape(N - 1, S, S)
    area = segment_areas(records, S)
    link = _filled(link_fill, (N - 1, S), np.int32)
    for k in range(N - 1):
        c = overlap[k, :n[k], :n[k + 1]].astype(np.int64)
        out = np.zeros(n[k], np.int32)
        if n[k] and n[k + 1]:
            fbest, bbest = c.argmax(axis=1), c.argmax(axis=0)   # (argmax: the first of equals, the smallest index)
            for a in range(n[k]):
                b = int(fbest[a])
                if c[a, b] > 0 and bbest[b] == a and int(c[a, b]) * 100 >= min_share * min(int(area[k, a]), int(area[k + 1, b])):
                    out[a] = b + 1
        link[k, :n[k]] = out
    return link


def _wrap(x):
    """an integer as int64 in two's complement"""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def segment_chain_ref(link, records, info, max_segments, max_tracks, ids_fill=None, tracks_fill=None):
    """link int32 [N - 1, S], records int64 [N, S, 12], info int64 [N, 4] -> (ids int32 [N, S], tracks int64 [max_tracks, 12],
    tinfo int64 [4]); ids [k, :n_k] and the first tinfo[1] track records are defined, the others keep the fills (or zeros)"""
    S = max_segments
    n = recorded_counts(info, S)
    N = len(n)
    _track_args(N, S, 0, max_tracks)
    link = np.asarray(link, np.int32).reshape(N - 1, S)
    records = np.asarray(records, np.int64).reshape(N, S, SEG_RECORD_FIELDS)
    ids = _filled(ids_fill, (N, S), np.int32)
    tracks = _filled(tracks_fill, (max_tracks, SEGTRACK_FIELDS), np.int64)
    recs = {}       # track id -> its record as Python integers
    length = {}     # (k, s) -> the length of its track up to map k
    ntracks = links = longest = 0
    for k in range(N):
        pred = {}
        if k:
            for a in range(int(n[k - 1]), 0, -1):   # (descending: the smallest a stays)
                b = int(link[k - 1, a - 1])
                if 1 <= b <= n[k]:
                    pred[b] = a
        for s in range(1, int(n[k]) + 1):
            r = [int(x) for x in records[k, s - 1]]
            if s not in pred:
                ntracks += 1
                t = ntracks
                length[k, s] = 1
                recs[t] = [k, s, 1, s, r[0], r[6], r[7], r[8], r[9], r[10], r[0], r[0]]
            else:
                t = int(ids[k - 1, pred[s] - 1])
                length[k, s] = length[k - 1, pred[s]] + 1
                links += 1
                q = recs[t]
                q[2], q[3] = length[k, s], s
                for i, f in ((4, 0), (5, 6), (6, 7), (7, 8), (8, 9), (9, 10)):
                    q[i] = _wrap(q[i] + r[f])
                q[10], q[11] = min(q[10], r[0]), max(q[11], r[0])
            ids[k, s - 1] = t
            longest = max(longest, length[k, s])
    for t in range(1, min(ntracks, max_tracks) + 1):
        tracks[t - 1] = recs[t]
    return ids, tracks, np.array([ntracks, min(ntracks, max_tracks), links, longest], np.int64)


def segment_relabel_ref(segments, ids, info, max_segments):
    """segments int32 [N, h, w], ids int32 [N, S] -> track_map int32 [N, h, w]: every entry written"""
    segments = np.asarray(segments, np.int32)
    N = segments.shape[0]
    _track_args(N, max_segments)
    ids = np.asarray(ids, np.int32).reshape(N, max_segments)
    n = recorded_counts(info, max_segments)
    out = np.zeros(segments.shape, np.int32)
    for k in range(N):
        s = segments[k].astype(np.int64)
        rec = (s >= 1) & (s <= n[k])
        out[k][rec] = ids[k][s[rec] - 1]
    return out


def segment_tracks_ref(segments, flow, records, info, max_segments, min_share, max_tracks, track_map=True, ids_fill=None,
                       tracks_fill=None):
    """the four steps in turn -> (ids, tracks, tinfo, track_map or None)"""
    overlap = segment_overlap_ref(segments, flow, info, max_segments)
    link = segment_link_ref(overlap, records, info, max_segments, min_share)
    ids, tracks, tinfo = segment_chain_ref(link, records, info, max_segments, max_tracks, ids_fill, tracks_fill)
    return ids, tracks, tinfo, segment_relabel_ref(segments, ids, info, max_segments) if track_map else None
