"""The host image readers and writers (of_dis_amd/csrc/host/image_io.cpp) on their own, on the CPU: the PNM and PNG decoders
against the arrays the files were written from (tests/png_files.py makes every path of the PNG decoder reachable), the gray
conversion against its formula, a corpus of malformed files that must each be refused with a message and a normal exit, two
deterministic sweeps (every prefix, every early byte), and the .flo / .pfm / .pgm writers and half_to_float against the
Python statements of the same formats.  All through tests/c/image_io_probe.cpp, a program without the HIP runtime:
OFDIS_IMAGE_IO_PROBE names another build of it (tools/host_sanitize.sh: AddressSanitizer + UBSan)."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import flow_images
import gen_synth
import png_files
from png_files import chunk, ihdr, png, png_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.environ.get("OFDIS_IMAGE_IO_PROBE") or os.path.join(ROOT, "of_dis_amd", "lib", "image_io_probe")

SIZES = [(1, 1), (1, 9), (13, 1), (7, 5), (64, 3)]      # (width, height)
FILTERS = [0, 1, 2, 3, 4, (4, 1, 3, 0, 2)]              # one type on every row, and a mix row by row
PALETTE = np.array([[(37 * k + 11) & 255, (91 * k + 5) & 255, (k * k + 3 * k) & 255] for k in range(256)], np.uint8)


def _probe(args):
    assert os.path.exists(PROBE), f"{PROBE} missing: python -m of_dis_amd.build"
    r = subprocess.run([PROBE] + args, capture_output=True, text=True, timeout=120)
    # (a sanitizer report ends the sanitized probe with a non-zero status and stands in stderr)
    assert r.returncode == 0, f"image_io_probe ended with status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return r.stdout.splitlines()


def read_all(tmp, items):
    """items: [(path, channels)] through ONE probe process.  Per item ("OK", w, h, c, bytes) or ("ERR", message)."""
    tmp = str(tmp)
    out = os.path.join(tmp, "decoded")
    os.makedirs(out, exist_ok=True)
    manifest = os.path.join(tmp, "manifest.txt")
    with open(manifest, "w") as f:
        f.writelines(f"{p} {c}\n" for p, c in items)
    lines = _probe(["read", manifest, out])
    assert len(lines) == len(items), lines[-3:]
    res = []
    for k, line in enumerate(lines):
        tag, _, rest = line.partition(" ")
        if tag == "OK":
            w, h, c = map(int, rest.split())
            with open(os.path.join(out, f"{k}.raw"), "rb") as f:
                res.append(("OK", w, h, c, f.read()))
        else:
            assert tag == "ERR", line
            res.append(("ERR", rest))
    return res


def read_files(tmp, blobs, channels=None):
    """blobs: {name: bytes} (or {name: (bytes, channels)}) written under tmp and read in one process: {name: result}"""
    items, names = [], []
    for name, blob in blobs.items():
        blob, c = blob if isinstance(blob, tuple) else (blob, channels)
        path = os.path.join(str(tmp), name)
        with open(path, "wb") as f:
            f.write(blob)
        items.append((path, c))
        names.append(name)
    return dict(zip(names, read_all(tmp, items)))


def assert_decodes(res, want, what):
    """the result of one read is exactly the array `want` ([h][w] or [h][w][3])"""
    assert res[0] == "OK", f"{what}: {res[1]}"
    h, w = want.shape[:2]
    c = 1 if want.ndim == 2 else 3
    assert res[1:4] == (w, h, c), f"{what}: {res[1:4]}"
    assert res[4] == np.ascontiguousarray(want).tobytes(), f"{what}: pixels differ"


def _samples(w, h, spp, seed):
    """smooth ramps plus noise: each filter's predictor is exercised with wrap-around in both directions"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (xx * 37 + yy * 101)[..., None] + np.arange(spp) * 50
    return ((base + rng.integers(0, 40, (h, w, spp))) & 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- PNG
def _png_cases():
    """{name: (file bytes, expected pixels)} -- expected = the array the file was written from, colour as B,G,R"""
    cases = {}
    for ctype in (0, 2, 3, 4, 6):
        pal = PALETTE if ctype == 3 else None
        for w, h in SIZES:
            s = _samples(w, h, png_files.SPP[ctype], 10 * w + h)
            for fi, filt in enumerate(FILTERS):
                cases[f"c{ctype}_{w}x{h}_f{fi}.png"] = (png(s, ctype, filt, pal), png_files.decoded(s, ctype, pal))
    s = _samples(7, 5, 3, 1)
    want = png_files.decoded(s, 2)
    anc = [chunk(b"gAMA", struct.pack(">I", 45455)), chunk(b"tEXt", b"Comment\0IDAT IHDR PLTE"), chunk(b"tIME", bytes(7))]
    cases["idat_many.png"] = (png(s, 2, FILTERS[5], idat_split=(1, 1, 0, 7, 3)), want)       # 2-byte zlib header split, an empty chunk
    cases["idat_bytewise.png"] = (png(s, 2, 4, idat_split=(1,) * 40), want)
    cases["idat_stored.png"] = (png(s, 2, 3, level=0), want)                                 # stored deflate blocks
    cases["anc_before.png"] = (png(s, 2, 1, extra=[("before_plte", anc[0]), ("before_idat", anc[1])]), want)
    cases["anc_between.png"] = (png(s, 2, 2, idat_split=(9,), extra=[("between_idat", anc[1])]), want)
    cases["anc_after.png"] = (png(s, 2, 3, extra=[("after_idat", anc[2] + anc[1])]), want)
    cases["anc_all.png"] = (png(s, 2, FILTERS[5], idat_split=(5, 0), extra=[("before_plte", anc[0]), ("before_idat", anc[2]),
                                                                           ("between_idat", anc[1]), ("after_idat", anc[0])]), want)
    cases["plte_in_rgb.png"] = (png(s, 2, 0, palette=PALETTE[:3]), want)                     # a suggested palette: allowed, unused
    cases["no_iend.png"] = (png(s, 2, 4)[:-12], want)
    for n in (1, 2, 256):
        idx = (_samples(13, 4, 1, n).astype(np.int64) % n).astype(np.uint8)
        cases[f"plte{n}.png"] = (png(idx, 3, 4, PALETTE[:n]), png_files.decoded(idx, 3, PALETTE[:n]))
    # a palette index beyond PLTE stays black
    idx = np.arange(16, dtype=np.uint8).reshape(2, 8, 1)
    cases["plte_beyond.png"] = (png(idx, 3, 0, PALETTE[:5]), png_files.decoded(idx, 3, PALETTE[:5]))
    assert not cases["plte_beyond.png"][1][0, 5:].any() and cases["plte_beyond.png"][1][0, 1:5].any()
    return cases


# what Pillow cannot be asked about: IDAT chunks that are not consecutive (the specification wants them so; this decoder
# gathers them wherever they stand)
NOT_FOR_PILLOW = ("anc_between.png", "anc_all.png")


@pytest.fixture(scope="module")
def png_cases(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("png")
    cases = _png_cases()
    res = read_files(tmp, {name: (blob, 1 if want.ndim == 2 else 3) for name, (blob, want) in cases.items()})
    return tmp, cases, res


def test_png_every_colour_type_filter_and_size(png_cases):
    _, cases, res = png_cases
    assert len(cases) == 5 * len(SIZES) * len(FILTERS) + 13
    for name, (_, want) in cases.items():
        assert_decodes(res[name], want, name)


def test_png_writer_agrees_with_pillow(png_cases):
    """the writer of this module is itself checked: Pillow decodes its files to the same arrays"""
    Image = pytest.importorskip("PIL.Image")
    tmp, cases, _ = png_cases
    for name, (_, want) in cases.items():
        if name in NOT_FOR_PILLOW:
            continue
        with Image.open(os.path.join(str(tmp), name)) as im:
            got = np.asarray(im.convert("L" if want.ndim == 2 else "RGB"))
        assert np.array_equal(got if want.ndim == 2 else got[..., ::-1], want), name


# ------------------------------------------------------------------------------------------- gray <-> colour conversion
def _colour_grid():
    """[513][512][3] R,G,B: a 64^3 grid over 0..255 (both ends included) and {0, 1, 254, 255}^3, the corners and their neighbours"""
    g = np.rint(np.linspace(0, 255, 64)).astype(np.uint8)
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    e = np.array([0, 1, 254, 255], np.uint8)
    corners = np.stack(np.meshgrid(e, e, e, indexing="ij"), -1).reshape(-1, 3)
    rgb = np.zeros((513 * 512, 3), np.uint8)
    rgb[:len(grid)] = grid
    rgb[len(grid):len(grid) + len(corners)] = corners
    return rgb.reshape(513, 512, 3)


def test_colour_to_gray_is_the_fixed_point_formula(tmp_path):
    rgb = _colour_grid()
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    want = ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)
    assert want[0, 0] == 0 and want.max() == 255  # (the weights sum to 2^14)
    rgba = np.concatenate([rgb, np.full((513, 512, 1), 77, np.uint8)], -1)
    pal_idx = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    pal = rgb.reshape(-1, 3)[1000:1000 + 256 * 997:997]
    pr, pg, pb = (pal[:, k].astype(np.int64) for k in range(3))
    res = read_files(tmp_path, {"grid.ppm": b"P6\n512 513\n255\n" + rgb.tobytes(), "grid.png": png(rgb, 2, 0, level=1),
                                "grid_rgba.png": png(rgba, 6, 1, level=1), "pal.png": png(pal_idx, 3, 0, pal)}, channels=1)
    for name in ("grid.ppm", "grid.png", "grid_rgba.png"):
        assert_decodes(res[name], want, name)
    assert_decodes(res["pal.png"], ((4899 * pr + 9617 * pg + 1868 * pb + 8192) >> 14).astype(np.uint8).reshape(16, 16), "pal.png")


def test_gray_to_colour_replicates(tmp_path):
    gray = np.arange(256, dtype=np.uint8).reshape(8, 32)
    want = np.repeat(gray[..., None], 3, -1)
    ga = np.stack([gray, gray[::-1]], -1)  # the alpha channel is dropped, not blended
    res = read_files(tmp_path, {"g.pgm": b"P5\n32 8\n255\n" + gray.tobytes(), "g.png": png(gray[..., None], 0, 2),
                                "ga.png": png(ga, 4, 3)}, channels=3)
    for name in res:
        assert_decodes(res[name], want, name)


# ------------------------------------------------------------------------------------------------------------- PNM
def _pnm(magic, w, h, raster, seps=(b"\n", b" ", b"\n"), last=b"\n", maxval=b"255"):
    return magic + seps[0] + b"%d" % w + seps[1] + b"%d" % h + seps[2] + maxval + last + raster


def _pnm_cases():
    """{name: (bytes, expected)}; P6 stores R,G,B, Image8 holds B,G,R"""
    cases = {}
    for magic, spp in ((b"P5", 1), (b"P6", 3)):
        tag = magic.decode()
        for w, h in [(1, 1), (2, 2), (5, 3), (64, 3)]:
            s = _samples(w, h, spp, 7 * w + h)
            want = s[..., 0] if spp == 1 else s[..., ::-1]
            cases[f"{tag}_{w}x{h}"] = (_pnm(magic, w, h, s.tobytes()), want)
        s = _samples(5, 3, spp, 3)
        want = s[..., 0] if spp == 1 else s[..., ::-1]
        raster = s.tobytes()
        for k, sep in enumerate((b" ", b"\t", b"\n", b"\r", b"\r\n", b" \t\r\n  ")):
            cases[f"{tag}_sep{k}"] = (_pnm(magic, 5, 3, raster, (sep, sep, sep), sep[:1]), want)
        # comments: after the magic number on its line, on lines of their own, empty, after the width, after the height (with
        # digits inside them), two in a row -- and, as Netpbm reads them, directly behind a token
        cases[f"{tag}_comments"] = (magic + b" # 9 9 255\n# made by hand\n#\n5 # width 7\n3 # height\n# 65535\n#again\n255\n" + raster, want)
        cases[f"{tag}_comment_abuts"] = (magic + b"#c\n5# width\n3# height\n255\n" + raster, want)
        cases[f"{tag}_trailing"] = (_pnm(magic, 5, 3, raster + b"\n# trailing bytes 1 2 3" + bytes(40)), want)
        cases[f"{tag}_leading_zeros"] = (magic + b"\n005 03\n0255\n" + raster, want)
        # ONE white-space byte ends the header: a raster that begins with white space keeps it ...
        ws = np.frombuffer(b"\n \t\r" + raster[4:], np.uint8).reshape(s.shape)
        cases[f"{tag}_ws_raster"] = (_pnm(magic, 5, 3, ws.tobytes()), ws[..., 0] if spp == 1 else ws[..., ::-1])
        # ... and of "255\r\n" the CR is that byte: the LF is the first sample, the last byte of the file is left over
        crlf = np.frombuffer((b"\n" + raster)[:len(raster)], np.uint8).reshape(s.shape)
        cases[f"{tag}_crlf"] = (magic + b"\r\n5 3\r\n255\r\n" + raster, crlf[..., 0] if spp == 1 else crlf[..., ::-1])
    return cases


@pytest.fixture(scope="module")
def pnm_cases(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pnm")
    cases = _pnm_cases()
    res = read_files(tmp, {name: (blob, 1 if want.ndim == 2 else 3) for name, (blob, want) in cases.items()})
    return tmp, cases, res


def test_pnm_headers_separators_comments_and_small_sizes(pnm_cases):
    _, cases, res = pnm_cases
    assert len(cases["P5_1x1"][0]) == 12 and len(cases["P5_2x2"][0]) == 15  # shorter than any PNG: read all the same
    for name, (_, want) in cases.items():
        assert_decodes(res[name], want, name)


def test_pnm_one_byte_rule_is_pillows(pnm_cases):
    """the byte after maxval as Pillow reads it (CR LF: the LF belongs to the raster), and the other headers with it"""
    Image = pytest.importorskip("PIL.Image")
    tmp, cases, _ = pnm_cases
    checked = 0
    for name, (_, want) in cases.items():
        if "comment_abuts" in name:  # (Pillow wants white space between a token and a comment)
            continue
        with Image.open(os.path.join(str(tmp), name)) as im:
            got = np.asarray(im.convert("L" if want.ndim == 2 else "RGB"))
        assert np.array_equal(got if want.ndim == 2 else got[..., ::-1], want), name
        checked += "crlf" in name
    assert checked == 2


# ---------------------------------------------------------------------------------------------------- malformed files
def _zraw(w, h, spp, ft=0):
    return b"".join(bytes([ft]) + bytes((x * 3 + y) & 255 for x in range(w * spp)) for y in range(h))


def _malformed():
    good_raw = _zraw(4, 3, 1)
    z = zlib.compress(good_raw)
    head, iend = png_files.SIGNATURE + ihdr(4, 3, 0), chunk(b"IEND", b"")
    big = 2 ** 31 - 1
    short_ihdr = struct.pack(">IIBB", 4, 3, 8, 0)[:8]  # width and height only
    corrupt = bytearray(z)
    corrupt[len(z) // 2] ^= 0x55
    m = {
        # --- the reader's first moments
        "empty": b"",
        "one_byte": b"P",
        "signature_only.png": png_files.SIGNATURE,
        "signature_and_half_a_chunk.png": head[:20],
        "not_an_image": b"GIF89a" + bytes(40),
        # --- PNG headers
        "huge_ihdr.png": png_raw(big, big, 2, good_raw),
        "huge_ihdr_rgba.png": png_raw(big, big, 6, good_raw),                # 4 (2^31-1)^2 + ...: past 64 bits
        "size_2_32.png": png_raw(65536, 65536, 0, good_raw),                 # 2^32 pixels: past 32 bits
        "size_2_32_rgba.png": png_raw(32768, 32768, 6, good_raw),            # 2^32 bytes a plane
        "size_negative.png": png_raw(0xFFFFFFFF, 0xFFFFFFFF, 0, good_raw),
        "width_2_31.png": png_raw(0x80000004, 3, 0, good_raw),               # (4 when the top bit is dropped)
        "zero_width.png": png_raw(0, 3, 0, good_raw),
        "zero_height.png": png_raw(4, 0, 0, good_raw),
        "short_ihdr.png": png_files.SIGNATURE + chunk(b"IHDR", short_ihdr) + chunk(b"IDAT", z) + iend,
        # (the four bytes where depth, colour type and the rest would stand are the CRC, which nobody checks: make them plausible)
        "short_ihdr_plausible.png": png_files.SIGNATURE + struct.pack(">I", 8) + b"IHDR" + short_ihdr + b"\x08\x00\x00\x00" + chunk(b"IDAT", z) + iend,
        "short_ihdr_ends_the_file.png": png_files.SIGNATURE + chunk(b"IDAT", z) + chunk(b"IHDR", short_ihdr),  # (the interlace byte: past the end)
        "short_ihdr_alone.png": png_files.SIGNATURE + chunk(b"IHDR", short_ihdr),
        "long_ihdr.png": png_files.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBBB", 4, 3, 8, 0, 0, 0, 0, 0)) + chunk(b"IDAT", z) + iend,
        "empty_ihdr.png": png_files.SIGNATURE + chunk(b"IHDR", b"") + chunk(b"IDAT", z) + iend + bytes(16),
        "missing_ihdr.png": png_files.SIGNATURE + chunk(b"IDAT", z) + iend + bytes(24),
        "idat_before_ihdr.png": png_files.SIGNATURE + chunk(b"IDAT", z) + ihdr(4, 3, 0) + iend,
        "two_ihdr.png": head + ihdr(2, 6, 0) + chunk(b"IDAT", z) + iend,
        "no_idat.png": head + chunk(b"tEXt", b"k\0" + bytes(30)) + iend,
        "colour_type_5.png": png_raw(4, 3, 5, good_raw),
        # --- chunks
        "chunk_past_end.png": head + struct.pack(">I", len(z) + 64) + b"IDAT" + z + iend,
        "chunk_length_2_31.png": head + struct.pack(">I", 0x7FFFFFFF) + b"IDAT" + z + iend,
        "chunk_length_2_32.png": head + struct.pack(">I", 0xFFFFFFFF) + b"IDAT" + z + iend,
        "chunk_length_wraps.png": head + struct.pack(">I", 0xFFFFFFF4) + b"IDAT" + z + iend,   # 12 + length = 0 in 32 bits
        "truncated_in_idat.png": (head + chunk(b"IDAT", z))[:-9],
        # --- the zlib stream
        "zlib_truncated.png": head + chunk(b"IDAT", z[:-5]) + iend,
        "zlib_header_only.png": head + chunk(b"IDAT", z[:2]) + iend,
        "zlib_empty.png": head + chunk(b"IDAT", b"") + iend,
        "zlib_corrupt.png": head + chunk(b"IDAT", bytes(corrupt)) + iend,
        "zlib_garbage.png": head + chunk(b"IDAT", bytes(range(7, 47))) + iend,
        "inflates_to_more.png": png_raw(4, 3, 0, good_raw + _zraw(4, 1, 1)),
        "inflates_to_one_more.png": png_raw(4, 3, 0, good_raw + b"\0"),
        "inflates_to_fewer.png": png_raw(4, 3, 0, good_raw[:-5]),
        "inflates_to_one_fewer.png": png_raw(4, 3, 0, good_raw[:-1]),
        "inflates_to_nothing.png": png_raw(4, 3, 0, b""),
        "zeros_for_a_large_image.png": png_raw(30000, 30000, 0, bytes(100000)),   # 0.9 GB asked for, 100 kB delivered
        # --- filters and palettes
        "filter_9.png": png_raw(4, 3, 0, _zraw(4, 2, 1) + _zraw(4, 1, 1, ft=9)),
        "filter_5.png": png_raw(4, 3, 0, _zraw(4, 3, 1, ft=5)),
        "filter_255.png": png_raw(4, 3, 2, _zraw(4, 3, 3, ft=255)),
        "palette_without_plte.png": png_raw(4, 3, 3, good_raw),
        "plte_empty.png": png_raw(4, 3, 3, good_raw, plte=b""),
        "plte_4_bytes.png": png_raw(4, 3, 3, good_raw, plte=bytes(4)),
        "plte_767_bytes.png": png_raw(4, 3, 3, good_raw, plte=bytes(767)),
        "plte_771_bytes.png": png_raw(4, 3, 3, good_raw, plte=bytes(771)),
        # --- PNM
        "width_20_digits.pgm": b"P5\n12345678901234567890 3\n255\n" + bytes(15),
        "width_2_32_plus_5.pgm": b"P5\n4294967301 3\n255\n" + bytes(15),       # 5 when 32 bits are kept
        "height_2_32_plus_3.pgm": b"P5\n5 4294967299\n255\n" + bytes(15),
        "maxval_2_32_plus_255.pgm": b"P5\n5 3\n4294967551\n" + bytes(15),
        "size_2_62.pgm": b"P5\n2147483647 2147483647\n255\n" + bytes(15),
        "size_2_32.ppm": b"P6\n65536 65536\n255\n" + bytes(48),                # 3 * 2^32 bytes
        "size_2_32_to_zero.pgm": b"P5\n65536 65536\n255\n" + bytes(15),        # w * h = 0 in 32 bits
        "maxval_100.pgm": b"P5\n5 3\n100\n" + bytes(15),
        "maxval_254.ppm": b"P6\n5 3\n254\n" + bytes(45),
        "maxval_0.pgm": b"P5\n5 3\n0\n" + bytes(15),
        "maxval_256.pgm": b"P5\n5 3\n256\n" + bytes(30),
        "maxval_65535.pgm": b"P5\n5 3\n65535\n" + bytes(30),
        "maxval_65535.ppm": b"P6\n5 3\n65535\n" + bytes(90),
        "plain_p2.pgm": b"P2\n2 2\n255\n1 2 3 4\n" + bytes(16),
        "plain_p3.ppm": b"P3\n1 1\n255\n1 2 3\n" + bytes(16),
        "p4_bitmap.pbm": b"P4\n8 8\n" + bytes(16),
        "raster_one_short.pgm": b"P5\n5 3\n255\n" + bytes(14),
        "raster_one_short.ppm": b"P6\n5 3\n255\n" + bytes(44),
        "header_only.pgm": b"P5\n5 3\n255\n",
        "header_without_end.pgm": b"P5\n5 3\n255",
        "no_maxval.pgm": b"P5\n5 3\n" + bytes(20),
        "no_numbers.pgm": b"P5\n# only a comment that never ends" + bytes(20),
        "negative_width.pgm": b"P5\n-5 3\n255\n" + bytes(15),
        "p5": b"P5",
    }
    return m


MALFORMED = _malformed()
# refused because the format is out of scope, not because the file is broken: the message is part of the contract
OUT_OF_SCOPE = {
    "png_16_bit.png": png_raw(4, 3, 0, _zraw(8, 3, 1), depth=16),
    "png_interlaced.png": png_raw(4, 3, 0, _zraw(4, 3, 1), interlace=1),
    "png_4_bit.png": png_raw(4, 3, 0, _zraw(2, 3, 1), depth=4),
    "png_1_bit_palette.png": png_raw(8, 3, 3, _zraw(1, 3, 1), plte=bytes(6), depth=1),
}


def _one(tmp_path, path, channels=1):
    (res,) = read_all(tmp_path, [(str(path), channels)])
    return res


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_file_is_refused_with_a_message(tmp_path, name):
    """a process of its own per file: the exit status is normal (checked by the runner), the answer is ERR and names the path"""
    path = tmp_path / name
    path.write_bytes(MALFORMED[name])
    for channels in (1, 3):
        res = _one(tmp_path, path, channels)
        assert res[0] == "ERR", f"{name} was read as {res[1:4]}"
        assert str(path) in res[1], res[1]


def test_unreadable_paths_are_refused_with_a_message(tmp_path):
    (tmp_path / "dir.png").mkdir()
    (tmp_path / "full_dir.pgm").mkdir()
    (tmp_path / "full_dir.pgm" / "a.pgm").write_bytes(b"P5\n1 1\n255\n\0")
    for name in ("dir.png", "full_dir.pgm", "nonexistent.png", "no_such_dir/a.pgm"):
        res = _one(tmp_path, tmp_path / name)
        assert res[0] == "ERR" and str(tmp_path / name) in res[1], (name, res)
    assert _one(tmp_path, tmp_path / "full_dir.pgm" / "a.pgm")[0] == "OK"


def test_maxval_below_255_and_out_of_scope_pngs_say_unsupported(tmp_path):
    res = read_files(tmp_path, dict(OUT_OF_SCOPE, **{k: MALFORMED[k] for k in ("maxval_100.pgm", "maxval_254.ppm")}), channels=1)
    for name, r in res.items():
        assert r[0] == "ERR" and str(tmp_path / name) in r[1], (name, r)
        assert "unsupported" in r[1] and "need 8-bit" in r[1], (name, r)
    assert "non-interlaced" in res["png_interlaced.png"][1]


# ------------------------------------------------------------------------------------------------------- the two sweeps
def _sweep_png():
    s = _samples(7, 5, 3, 99)
    blob = png(s, 2, FILTERS[5], idat_split=(20,), extra=[("before_idat", chunk(b"tEXt", b"k\0v")), ("after_idat", chunk(b"tIME", bytes(7)))])
    end_of_idat = blob.rindex(b"IDAT") - 4
    end_of_idat += 12 + struct.unpack(">I", blob[end_of_idat:end_of_idat + 4])[0]
    assert blob.count(b"IDAT") == 2 and 64 < end_of_idat < len(blob) - 12
    return blob, png_files.decoded(s, 2), end_of_idat


def _assert_prefixes(tmp_path, blob, want, complete_from, channels):
    res = read_files(tmp_path, {f"{n:04d}": blob[:n] for n in range(len(blob))}, channels=channels)
    for n in range(len(blob)):
        r = res[f"{n:04d}"]
        if n < complete_from:
            assert r[0] == "ERR", f"the first {n} of {len(blob)} bytes were read as {r[1:4]}"
        elif r[0] == "OK":
            assert_decodes(r, want, f"the first {n} bytes")
    return res


def test_every_prefix_of_a_png(tmp_path):
    blob, want, end_of_idat = _sweep_png()
    assert_decodes(_one(tmp_path, _write(tmp_path / "whole.png", blob), 3), want, "the whole file")
    res = _assert_prefixes(tmp_path, blob, want, end_of_idat, 3)
    assert res[f"{end_of_idat:04d}"][0] == "OK"  # (IEND is not insisted on: everything the pixels need is there)


def test_every_prefix_of_a_pgm(tmp_path):
    s = _samples(7, 5, 1, 98)
    head = b"P5\n# c\n7 5\n255\n"
    blob = head + s.tobytes() + b"trailing"
    res = _assert_prefixes(tmp_path, blob, s[..., 0], len(head) + 35, 1)
    assert all(res[f"{n:04d}"][0] == "OK" for n in range(len(head) + 35, len(blob)))


def _write(path, blob):
    path.write_bytes(blob)
    return path


def test_every_early_byte_of_a_png_replaced(tmp_path):
    """each of the first 64 bytes (signature, IHDR, the text chunk, the head of the first IDAT) as 0x00, 0xFF and its complement:
    whatever the answer, the process ends normally and an OK comes with exactly w * h * c bytes"""
    blob, want, _ = _sweep_png()
    blobs = {}
    for k in range(64):
        for v in (0x00, 0xFF, blob[k] ^ 0xFF):
            if v != blob[k]:
                blobs[f"{k:02d}_{v:02x}"] = blob[:k] + bytes([v]) + blob[k + 1:]
    assert len(blobs) >= 2 * 64
    answers = set()
    for channels in (1, 3):
        for name, r in read_files(tmp_path, blobs, channels=channels).items():
            answers.add(r[0])
            if r[0] == "OK":
                assert r[1] > 0 and r[2] > 0 and r[3] == channels and len(r[4]) == r[1] * r[2] * r[3], (name, r[1:4], len(r[4]))
            else:
                assert str(tmp_path / name) in r[1]
    assert answers == {"OK", "ERR"}  # (a changed CRC byte is still the image; a changed signature is not)


# ------------------------------------------------------------------------------------------------------------ writers
def _special_floats(n, seed):
    """n float32 values as bit patterns: NaNs of both signs, quiet and signalling, with payloads; infinities; both zeros;
    denormals; the largest and smallest normals; ordinary values"""
    special = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFBADBAD, 0x7F800000, 0xFF800000,
                        0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x7F7FFFFF,
                        0xFF7FFFFF, 0x3F800000, 0xBF800000], np.uint32)
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    k = min(n, len(special))
    bits[rng.permutation(n)[:k]] = special[(np.arange(k) + seed) % len(special)]
    return bits


WRITER_SIZES = [(1, 1), (5, 3), (64, 16)]


def _run_writes(tmp_path, lines):
    manifest = tmp_path / "writes.txt"
    manifest.write_text("".join(line + "\n" for line in lines))
    out = _probe(["write", str(manifest)])
    assert len(out) == len(lines)
    return out


def test_flo_and_pfm_writers_are_the_python_writers_byte_for_byte(tmp_path):
    lines, want = [], {}
    for w, h in WRITER_SIZES:
        for kind, ch in (("flo", 2), ("pfm", 1)):
            for seed in range(3 if w == 1 else 1):  # (1x1: a few of the special values each)
                bits = _special_floats(w * h * ch, 17 * seed + w).reshape((h, w, 2) if ch == 2 else (h, w))
                tag = f"{kind}_{w}x{h}_{seed}"
                (tmp_path / f"{tag}.raw").write_bytes(bits.tobytes())
                lines.append(f"{kind} {tmp_path}/{tag}.raw {w} {h} {tmp_path}/{tag}.out")
                py = str(tmp_path / f"{tag}.py")
                if kind == "flo":
                    flow_images.write_flo(py, bits.view(np.float32))
                    body = bits.tobytes()
                    head = b"PIEH" + struct.pack("<ii", w, h)
                else:
                    flow_images.write_pfm(py, bits.view(np.float32))
                    body = (bits[::-1] ^ np.uint32(0x80000000)).tobytes()  # rows bottom-up, the sign bit flipped, nothing else
                    head = b"Pf\n%d %d\n-1.000000\n" % (w, h)
                with open(py, "rb") as f:
                    assert f.read() == head + body, f"{tag}: the Python writer is not the stated format"
                want[tag] = head + body
    assert _run_writes(tmp_path, lines) == ["OK"] * len(lines)
    for tag, blob in want.items():
        assert (tmp_path / f"{tag}.out").read_bytes() == blob, tag


def test_pgm_plane_writer_both_widths(tmp_path):
    lines, want = [], {}
    rng = np.random.default_rng(5)
    for w, h in WRITER_SIZES:
        for sb, dtype in ((1, np.uint8), (2, np.uint16)):
            for channels in (1, 2):
                a = rng.integers(0, 256 ** sb, (h, w, channels)).astype(dtype)
                a.flat[0], a.flat[-1] = 256 ** sb - 1, 0x0102 % 256 ** sb  # (0x0102: the byte order shows)
                (tmp_path / f"s{sb}_{w}x{h}_{channels}.raw").write_bytes(a.tobytes())
                for channel in range(channels):
                    tag = f"s{sb}_{w}x{h}_{channels}_{channel}"
                    lines.append(f"pgm {tmp_path}/s{sb}_{w}x{h}_{channels}.raw {w} {h} {channels} {channel} {sb} {tmp_path}/{tag}.out")
                    plane = a[..., channel]
                    if sb == 1:  # tools/gen_synth.py writes this file
                        gen_synth.write_pgm(str(tmp_path / f"{tag}.py"), plane)
                        want[tag] = (tmp_path / f"{tag}.py").read_bytes()
                        assert want[tag] == b"P5\n%d %d\n255\n" % (w, h) + plane.tobytes()
                    else:        # 16 bits: most significant byte first, as PNM defines (--link u16)
                        want[tag] = b"P5\n%d %d\n65535\n" % (w, h) + plane.astype(">u2").tobytes()
    assert _run_writes(tmp_path, lines) == ["OK"] * len(lines)
    for tag, blob in want.items():
        assert (tmp_path / f"{tag}.out").read_bytes() == blob, tag
    # and the reader takes the 8-bit planes back
    tag = "s1_5x3_2_1"
    r = _one(tmp_path, tmp_path / f"{tag}.out")
    assert r[0] == "OK" and r[1:4] == (5, 3, 1) and want[tag].endswith(r[4])


def test_16_bit_pgm_planes_read_back_in_pillow(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    a = np.arange(15, dtype=np.uint16).reshape(3, 5) * 4369 + 258
    (tmp_path / "a.raw").write_bytes(a.tobytes())
    assert _run_writes(tmp_path, [f"pgm {tmp_path}/a.raw 5 3 1 0 2 {tmp_path}/a.out"]) == ["OK"]
    os.rename(tmp_path / "a.out", tmp_path / "a.pgm")
    with Image.open(tmp_path / "a.pgm") as im:
        assert np.array_equal(np.asarray(im).astype(np.uint16), a)


def test_writers_report_an_unwritable_path(tmp_path):
    (tmp_path / "f.raw").write_bytes(bytes(8))
    nowhere = f"{tmp_path}/no_such_dir/out"
    is_dir = str(tmp_path)
    lines = [f"{verb} {tmp_path}/f.raw 1 1 {args}{out}" for out in (nowhere, is_dir) for verb, args in (("flo", ""), ("pfm", ""), ("pgm", "1 0 1 "), ("pgm", "1 0 2 "))]
    out = _run_writes(tmp_path, lines)
    for line, answer in zip(lines, out):
        assert answer.startswith("ERR ") and line.split()[-1] in answer, (line, answer)
    assert not os.path.exists(nowhere)


def test_half_to_float_all_bit_patterns(tmp_path):
    h = np.arange(65536, dtype=np.uint16)
    (tmp_path / "h.raw").write_bytes(h.tobytes())
    assert _run_writes(tmp_path, [f"half {tmp_path}/h.raw 65536 {tmp_path}/f.raw"]) == ["OK"]
    got = np.frombuffer((tmp_path / "f.raw").read_bytes(), np.uint32)
    want = h.view(np.float16).astype(np.float32).view(np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} patterns differ, first 0x{h[bad[0]]:04x}: 0x{got[bad[0]]:08x}, numpy 0x{want[bad[0]]:08x}"
    # numpy's conversion is itself the IEEE widening: exact values, NaN payloads moved up by 13 bits, signs kept
    e, m = (h.astype(np.int64) >> 10) & 31, h.astype(np.int64) & 1023
    finite = e < 31
    val = np.where(e == 0, m * 2.0 ** -24, (1024 + m) * 2.0 ** (e - 25.0)) * np.where(h & 0x8000, -1.0, 1.0)
    assert np.array_equal(got.view(np.float32)[finite].astype(np.float64), val[finite])
    assert np.array_equal(got[finite] >> 31, (h[finite] >> 15).astype(np.uint32))
    assert np.array_equal(got[~finite], ((h[~finite].astype(np.uint32) & 0x8000) << 16) | 0x7F800000 | (m[~finite].astype(np.uint32) << 13))
