"""Natural images for the parity tests.

Every other parity input of this repository is synthetic (tools/gen_synth.py).  These are a few photographs stored under
tests/golden/natural/ (see the README there for where they come from): a real Middlebury 2014 stereo pair,
`motorcycle_left.png` / `motorcycle_right.png`, with its ground-truth disparity, and four single photographs.
tests/golden/natural.json holds the SHA-256 of each input as decoded here and of the reference build's output for it (made by
tests/golden/make_natural.py), so that the CPU restatement is pinned on photographs as well.
"""
import hashlib
import lzma
import os

import numpy as np


DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "natural")


def find(name):
    p = os.path.join(DIR, name)
    return p if os.path.exists(p) else None


def pack_f32(arr, path):
    """A float32 image stored losslessly in about two thirds of the bytes np.savez_compressed needs (smooth fields such as a
    disparity map): the bit patterns as int32 differences down the columns, split into four byte planes, xz-compressed
    behind an 8-byte header (rows, columns as little-endian uint32).  load_f32 returns the same bits."""
    a = np.ascontiguousarray(arr, dtype=np.float32)
    bits = a.view(np.int32).astype(np.int64)
    delta = np.diff(bits, axis=0, prepend=0).astype("<i4")
    planes = np.frombuffer(delta.tobytes(), np.uint8).reshape(-1, 4).T.tobytes()
    head = np.array(a.shape, "<u4").tobytes()
    filt = [{"id": lzma.FILTER_LZMA2, "preset": 9 | lzma.PRESET_EXTREME, "lc": 4, "pb": 2}]
    with open(path, "wb") as f:
        f.write(lzma.compress(head + planes, format=lzma.FORMAT_XZ, filters=filt))


def load_f32(path):
    with open(path, "rb") as f:
        raw = lzma.decompress(f.read())
    h, w = (int(v) for v in np.frombuffer(raw[:8], "<u4"))
    delta = np.frombuffer(raw[8:], np.uint8).reshape(4, h * w).T.copy().view("<i4").reshape(h, w)
    return np.cumsum(delta, axis=0, dtype=np.int32).view(np.float32)  # (int32 sums wrap: the exact inverse of the differences)


def load_rgb(name):
    """(h, w, 3) uint8, R G B, or None when the file or a decoder is missing."""
    p = find(name)
    if p is None:
        return None
    try:
        from PIL import Image
    except Exception:
        return None
    return np.ascontiguousarray(np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8))


def to_channels(rgb, channels):
    """What the run_OF_* binaries hand to the pipeline for a colour file: B G R for the RGB binaries, OpenCV's fixed-point
    BGR2GRAY for the gray ones (of_dis_amd/csrc/host/image_io.cpp; run_dense.cpp:204-222 via cv::imread)."""
    if channels == 3:
        return np.ascontiguousarray(rgb[..., ::-1])
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def similarity_warp(img, angle_deg, scale, tx, ty):
    """The second frame of a pair made from ONE photograph: img resampled (bilinear, float64, replicate border) under a
    rotation + scale about the centre + translation; returns (second image uint8, ground-truth flow (h, w, 2) f32 of the
    first frame's pixels)."""
    h, w = img.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    a = np.deg2rad(angle_deg)
    c, s = np.cos(a) * scale, np.sin(a) * scale
    # forward map of frame-1 pixels: p2 = R (p1 - centre) + centre + t
    fx = c * (xx - cx) - s * (yy - cy) + cx + tx
    fy = s * (xx - cx) + c * (yy - cy) + cy + ty
    flow = np.stack([fx - xx, fy - yy], -1).astype(np.float32)
    # frame 2 at pixel q shows frame 1 at R^-1 (q - centre - t) + centre
    det = c * c + s * s
    qx, qy = xx - cx - tx, yy - cy - ty
    sx = (c * qx + s * qy) / det + cx
    sy = (-s * qx + c * qy) / det + cy
    sx, sy = np.clip(sx, 0, w - 1), np.clip(sy, 0, h - 1)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = sx - x0, sy - y0
    src = img.astype(np.float64)
    if src.ndim == 2:
        src = src[..., None]
    out = ((1 - ay) * (1 - ax))[..., None] * src[y0, x0] + ((1 - ay) * ax)[..., None] * src[y0, x1] + \
        (ay * (1 - ax))[..., None] * src[y1, x0] + (ay * ax)[..., None] * src[y1, x1]
    out = np.clip(np.rint(out), 0, 255).astype(np.uint8)
    return (out[..., 0] if img.ndim == 2 else out), flow


# name -> how to make the pair; every entry yields (first, second) as RGB uint8 arrays plus optional ground truth
def pair(name):
    """Returns (rgb_a, rgb_b, truth) or None.  truth: dict with 'flow' (h,w,2) or 'disparity' (h,w; inf = unknown)."""
    if name == "motorcycle":
        a, b = load_rgb("motorcycle_left.png"), load_rgb("motorcycle_right.png")
        if a is None or b is None:
            return None
        truth = {}
        p = find("motorcycle_disp.f32.xz")
        if p is not None:
            truth["disparity"] = load_f32(p)
        return a, b, truth
    src = {"china": ("china.png", 1.2, 1.015, 4.3, -2.6), "astronaut": ("astronaut.png", -2.0, 0.99, -6.4, 3.2),
           "coffee": ("coffee.png", 0.8, 1.0, 9.5, 1.25), "chelsea": ("chelsea.png", -0.6, 1.02, -3.1, -4.7)}.get(name)
    if src is None:
        return None
    a = load_rgb(src[0])
    if a is None:
        return None
    b, flow = similarity_warp(a, *src[1:])
    return a, b, {"flow": flow}


PAIRS = ("motorcycle", "china", "astronaut", "coffee", "chelsea")


def sha(arr):
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()
