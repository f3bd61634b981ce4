"""A PNG writer of struct and zlib, for the tests of the host image reader (of_dis_amd/csrc/host/image_io.cpp): every colour
type, every scanline filter, IDAT split at will, ancillary chunks anywhere -- the paths of the decoder that an ordinary
encoder reaches only when it chooses to -- and the pieces to put malformed files together from.  8-bit samples, no interlace.

    png(samples, ctype, filters=..., palette=..., idat_split=..., extra=...)   -> bytes
    png_raw(w, h, ctype, raw, ...)     -> bytes: the header fields and the uncompressed data as given, right or wrong
    decoded(samples, ctype, palette)   -> what Image8 holds for that file: [h][w] gray or [h][w][3] in B,G,R order
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
SPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}  # colour type -> samples per pixel (gray, RGB, palette index, gray+alpha, RGBA)


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def ihdr(w, h, ctype, depth=8, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))


def _shift(row, n):  # the sample n bytes to the left, 0 before the first pixel
    out = np.zeros_like(row)
    out[n:] = row[:-n] if n < row.size else 0
    return out


def filter_row(cur, up, bpp, ft):
    """One scanline under filter type ft (PNG specification, 9.2): cur and up are the unfiltered bytes as int arrays."""
    a, b, c = _shift(cur, bpp), up, _shift(up, bpp)
    if ft == 0:
        pred = 0
    elif ft == 1:
        pred = a
    elif ft == 2:
        pred = b
    elif ft == 3:
        pred = (a + b) // 2
    else:
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return bytes([ft]) + ((cur - pred) & 255).astype(np.uint8).tobytes()


def scanlines(samples, filters):
    """The uncompressed image data: per row the filter byte and the filtered samples.  filters: one type for every row or a
    sequence taken round-robin."""
    h = samples.shape[0]
    bpp = samples.shape[2]
    rows = samples.reshape(h, -1).astype(np.int64)
    if isinstance(filters, int):
        filters = [filters]
    up = np.zeros_like(rows[0])
    out = []
    for y in range(h):
        out.append(filter_row(rows[y], up, bpp, filters[y % len(filters)]))
        up = rows[y]
    return b"".join(out)


def split(data, sizes):
    """data cut into pieces of the given sizes (0 = an empty piece), the rest in a last one"""
    pieces, pos = [], 0
    for n in sizes:
        pieces.append(data[pos:pos + n])
        pos += n
    pieces.append(data[pos:])
    return pieces


def png(samples, ctype, filters=0, palette=None, idat_split=(), extra=(), level=6):
    """samples: uint8 [h][w][SPP[ctype]].  palette: uint8 [n][3] (R,G,B), written when given.  idat_split: sizes of the first
    IDAT chunks (split).  extra: ancillary chunks as (position, bytes), position one of "before_plte", "before_idat",
    "between_idat" (after the first IDAT chunk), "after_idat"."""
    samples = np.asarray(samples, np.uint8)
    h, w, spp = samples.shape
    assert spp == SPP[ctype]
    at = lambda where: b"".join(c for pos, c in extra if pos == where)
    out = [SIGNATURE, ihdr(w, h, ctype), at("before_plte")]
    if palette is not None:
        out.append(chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes()))
    out.append(at("before_idat"))
    for k, piece in enumerate(split(zlib.compress(scanlines(samples, filters), level), idat_split)):
        out.append(chunk(b"IDAT", piece))
        if k == 0:
            out.append(at("between_idat"))
    out += [at("after_idat"), chunk(b"IEND", b"")]
    return b"".join(out)


def png_raw(w, h, ctype, raw, plte=None, depth=8, interlace=0):
    """a PNG around the given UNCOMPRESSED image data (whatever it holds) and IHDR fields (whatever they claim)"""
    return SIGNATURE + ihdr(w, h, ctype, depth, interlace) + (chunk(b"PLTE", plte) if plte is not None else b"") + \
        chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b"")


def decoded(samples, ctype, palette=None):
    samples = np.asarray(samples, np.uint8)
    if ctype in (0, 4):
        return samples[..., 0].copy()
    if ctype == 3:
        table = np.zeros((256, 3), np.uint8)  # an index beyond PLTE reads as black
        table[:len(palette)] = palette
        return table[samples[..., 0]][..., ::-1].copy()
    return samples[..., 2::-1].copy() if ctype == 6 else samples[..., ::-1].copy()
