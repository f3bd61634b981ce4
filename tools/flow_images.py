"""Optical flow (or stereo disparity) of image pairs from Python, through the library's batch context -- what the run_OF_* /
run_DE_* binaries do (run_dense.cpp:185-431), for a list of pairs at once and without PyTorch: decode with PIL, upload the
8-bit frames, pad + pyramid + Sobel on the device, the hot path, x 2^lv_l upsample + crop on the device, write Middlebury .flo
(.pfm with --stereo).

    python tools/flow_images.py [--rgb] [--stereo [--lr [--fill MODE]]] [--op 1..4] [--fused] [--reverse] img1a img1b out1.flo [img2a img2b out2.flo ...]
    python tools/flow_images.py --sequence [--rgb] [--op 1..4] [--fused] [--reverse [--tracks STRIDE]
                                [--dense-tracks STRIDE[:WINDOW[:MIN_EIG[:MAX_LEN]]]
                                 [--track-select [MIN_LEN[:MIN_STD:MAX_STD:MAX_STEP:SHARE[:MIN_CAMERA]]] [--global-motion]]
                                 [--descriptors N:NXY:NT:MIN_FLOW]]]
                                img0 img1 ... imgN stem

All pairs must have one size.  --fused selects the FMA / fast-reciprocal arithmetic contract (default: the exact one, bit for
bit what run_OF_INT / run_OF_RGB write).  --reverse (optical flow only) also writes, next to <stem>.flo, the reverse flow
<stem>.rev.flo (second image to first) and the forward-backward consistency masks <stem>.mask.pgm / <stem>.rev.mask.pgm
(binary PGM, maxval 2, the raw codes: 0 consistent, 1 inconsistent, 2 target outside the image; ofdis_batch_upsample_bidir
with the default alpha 0.01 and beta 0.5).  --stereo --lr (the third argument of a pair is then a NAME, not a file) writes both
views of a stereo pair through an OFDIS_BATCH_STEREO_LR context and ofdis_batch_upsample_lr: <name>_left.pfm and
<name>_right.pfm (disparity magnitudes as Middlebury stores them, rows bottom-up, +inf = unknown) and the left-right masks
<name>_left_mask.pgm / <name>_right_mask.pgm (the same codes).  --fill none | invalidate | background (default none) says what
happens to the pixels the masks flag (ofdis_disparity_fill).  --sequence (optical flow only, --reverse allowed): the arguments
are the N + 1 frames of a clip and a stem; the flow from frame k to frame k + 1 goes to <stem>_<k as 000>.flo.  Every frame is
uploaded and built once, into an OFDIS_BATCH_SEQUENCE context (ofdis_batch_build_pyramids_u8_seq); the files are the ones the
pair-wise call writes for (img0, img1), (img1, img2), ...  --sequence --reverse --tracks STRIDE also writes the trajectories of
the grid of that stride seeded at frame 0 (ofdis_batch_track_points with the default alpha and beta): <stem>_tracks.npy,
float32 [N + 1][points][2] (x, y; NaN where a track has ended), and <stem>_counts.npy, int32 [points].  --sequence --reverse
--dense-tracks STRIDE[:WINDOW[:MIN_EIG[:MAX_LEN]]] (defaults 2, 0 and 15) writes the dense trajectories of the clip
(ofdis_batch_dense_tracks: the textured centres of a grid of that stride, the cells that lose their track seeded again in every
frame, a track at most MAX_LEN + 1 frames long): <stem>_dtracks.npy, float32 [Lmax + 1][tracks][2], step-major (entry [j][i] is
track i in frame start[i] + j; NaN beyond its length), <stem>_dstart.npy and <stem>_dlen.npy, int32 [tracks].  With
--descriptors N:NXY:NT:MIN_FLOW (needs --dense-tracks) the descriptors of those tracks follow (ofdis_track_descriptors on the
forward flows the run writes: an N x N window in NXY x NXY x NT cells, flows below MIN_FLOW in HOF's ninth bin):
<stem>_dhist.npy, uint32 [tracks][33 * NXY^2 * NT] (HOG, HOF, MBHx, MBHy: of_dis_amd/tracking.py descriptor_layout), and
<stem>_dshape.npy, float32 [tracks][Lmax][2].  --track-select [MIN_LEN[:MIN_STD:MAX_STD:MAX_STEP:SHARE[:MIN_CAMERA]]] (needs
--dense-tracks; defaults 0, sqrt(3), 50, 20, 0.7 and 1: ofdis_track_select_defaults) takes out the tracks that are too short, not
finite, static, erratic or one jump (ofdis_track_select) and, with --global-motion, those that move only as the camera does under
the clip's affine models (ofdis_batch_global_motion with the forward mask): <stem>_dcode.npy, uint8 [tracks], the code of every
track (0 kept; of_dis_amd/tracking.py TS_NAMES), and <stem>_dindex.npy, int32 [kept], their slots.  The three track files and
the descriptors then hold the kept tracks only."""
import itertools
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from of_dis_amd import capi, tracking  # noqa: E402
from of_dis_amd.params import oppoint, padded_size  # noqa: E402


def load(path, channels):
    """What the binaries hand to the pipeline: B G R for the RGB ones, OpenCV's fixed-point BGR2GRAY for the gray ones
    (of_dis_amd/csrc/host/image_io.cpp)."""
    from PIL import Image
    im = Image.open(path)
    if channels == 1 and im.mode in ("L", "1", "I;16"):
        return np.ascontiguousarray(np.asarray(im.convert("L"), dtype=np.uint8))
    rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
    if channels == 3:
        return np.ascontiguousarray(rgb[..., ::-1])
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def write_flo(path, flow):
    h, w = flow.shape[:2]
    with open(path, "wb") as f:
        f.write(b"PIEH" + struct.pack("<ii", w, h))
        f.write(np.ascontiguousarray(flow, np.float32).tobytes())


def write_pfm(path, disp):  # run_dense.cpp:60-81: rows bottom-up, values negated, little endian
    h, w = disp.shape[:2]
    with open(path, "wb") as f:
        f.write(b"Pf\n%d %d\n-1.000000\n" % (w, h))
        f.write(np.ascontiguousarray(-disp[::-1], np.float32).tobytes())


def write_pfm_magnitude(path, disp, sign):
    """sign * disp >= 0 (left view: -1, right view: +1), rows bottom-up, little endian; an invalidated pixel stays +inf"""
    h, w = disp.shape[:2]
    mag = np.where(np.isinf(disp), np.float32(np.inf), np.float32(sign) * disp).astype(np.float32)
    with open(path, "wb") as f:
        f.write(b"Pf\n%d %d\n-1.000000\n" % (w, h))
        f.write(np.ascontiguousarray(mag[::-1]).tobytes())


def write_pgm(path, mask):
    h, w = mask.shape
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n2\n" % (w, h))
        f.write(np.ascontiguousarray(mask, np.uint8).tobytes())


def main(argv):
    opts = {"--rgb": False, "--stereo": False, "--fused": False, "--reverse": False, "--lr": False, "--sequence": False,
            "--global-motion": False}
    op = 2
    fill = "none"
    track_stride = 0
    dense = None
    desc = None
    select = None
    args = []
    it = iter(argv)
    while True:
        a = next(it, None)
        if a is None:
            break
        if a in opts:
            opts[a] = True
        elif a == "--op":
            op = int(next(it))
        elif a == "--fill":
            fill = next(it)
        elif a == "--tracks":
            track_stride = int(next(it))
        elif a == "--dense-tracks":
            try:
                dense = [int(x) for x in next(it).split(":")]
            except ValueError:
                dense = []
            if not 1 <= len(dense) <= 4:
                sys.exit("--dense-tracks STRIDE[:WINDOW[:MIN_EIG[:MAX_LEN]]]")
            dense += [2, 0, 15][len(dense) - 1:]
        elif a == "--track-select":        # the values are optional: what follows is one only if it reads as numbers
            spec = next(it, None)
            try:
                values = [float(x) for x in spec.split(":")] if spec is not None else []
            except ValueError:
                values, it = [], itertools.chain([spec], it)
            if len(values) not in (0, 1, 5, 6) or (values and not values[0].is_integer()):
                sys.exit("--track-select [MIN_LEN[:MIN_STD:MAX_STD:MAX_STEP:SHARE[:MIN_CAMERA]]]")
            names = ("min_len", "min_std", "max_std", "max_step", "max_step_share", "min_camera")
            select = {k: int(v) if k == "min_len" else v for k, v in zip(names, values)}
        elif a == "--descriptors":
            try:
                n, nxy, nt, min_flow = next(it).split(":")
                desc = [int(n), int(nxy), int(nt), float(min_flow)]
            except ValueError:
                sys.exit("--descriptors N:NXY:NT:MIN_FLOW")
        else:
            args.append(a)
    if track_stride < 0 or (track_stride and not (opts["--sequence"] and opts["--reverse"])):
        sys.exit("--tracks STRIDE (>= 1) needs --sequence --reverse")
    if dense and not (opts["--sequence"] and opts["--reverse"]):
        sys.exit("--dense-tracks needs --sequence --reverse")
    if desc and not dense:
        sys.exit("--descriptors needs --dense-tracks")
    if select is not None and not dense:
        sys.exit("--track-select needs --dense-tracks")
    if opts["--global-motion"] and select is None:
        sys.exit("--global-motion needs --track-select")
    stem = args[-1] if args else None
    if opts["--sequence"]:
        if opts["--stereo"]:
            sys.exit("--sequence: a stereo pair is not a sequence")
        if len(args) < 3:
            sys.exit(__doc__)
        args = [x for k in range(len(args) - 2) for x in (args[k], args[k + 1], f"{args[-1]}_{k:03d}.flo")]
    if not args or len(args) % 3:
        sys.exit(__doc__)
    if opts["--reverse"] and opts["--stereo"]:
        sys.exit("--reverse: there is no reverse direction in stereo mode; the right view of a stereo pair is --lr")
    fills = {"none": capi.FILL_NONE, "invalidate": capi.FILL_INVALIDATE, "background": capi.FILL_BACKGROUND}
    if opts["--lr"] and not opts["--stereo"]:
        sys.exit("--lr needs --stereo")
    if fill not in fills or (fill != "none" and not opts["--lr"]):
        sys.exit("--fill none | invalidate | background, with --stereo --lr")
    noc = 3 if opts["--rgb"] else 1
    trip = [args[k:k + 3] for k in range(0, len(args), 3)]
    frames_a = [load(t[0], noc) for t in trip]
    frames_b = [load(trip[-1][1], noc)] if opts["--sequence"] else [load(t[1], noc) for t in trip]
    h, w = frames_a[0].shape[:2]
    if any(f.shape != frames_a[0].shape for f in frames_a + frames_b):
        sys.exit("all images must have one size")
    capi.set_tuning(contract=1 if opts["--fused"] else 0)
    p = oppoint(op, w, h, noc=noc).copy(selectmode=2 if opts["--stereo"] else 1)
    p.width, p.height = padded_size(w, h, p.sc_f)
    b = capi.Batch(p, len(trip), reverse=opts["--reverse"], stereo_lr=opts["--lr"], sequence=opts["--sequence"])
    da, db = capi.Dev(np.stack(frames_a + frames_b if opts["--sequence"] else frames_a)), capi.Dev(np.stack(frames_b))
    if opts["--sequence"]:  # the clip's frames, each once
        b.build_pyramids_u8_seq(da.ptr, w, h)
    else:
        b.build_pyramids_u8(da.ptr, db.ptr, w, h)
    b.run()
    if opts["--lr"]:                 # both views and both masks in one launch
        left, right, mask_l, mask_r = b.upsample_lr(w, h, fills[fill])
        b.close()
        da.free()
        db.free()
        for k, t in enumerate(trip):
            write_pfm_magnitude(t[2] + "_left.pfm", left[k], -1)
            write_pfm_magnitude(t[2] + "_right.pfm", right[k], 1)
            write_pgm(t[2] + "_left_mask.pgm", mask_l[k])
            write_pgm(t[2] + "_right_mask.pgm", mask_r[k])
            print(f"{t[2]}_left.pfm, _right.pfm, _left_mask.pgm, _right_mask.pgm: {w}x{h}, fill {fill}, consistent "
                  f"{np.mean(mask_l[k] == 0):.3f} / {np.mean(mask_r[k] == 0):.3f} of the pixels")
        return
    if track_stride:                 # straight from the level flows; the full-resolution flows below are for the files only
        tracks, counts = b.track_points(tracking.grid_seeds(w, h, track_stride), w, h)
        np.save(stem + "_tracks.npy", tracks)
        np.save(stem + "_counts.npy", counts)
        print(f"{stem}_tracks.npy, _counts.npy: {len(counts)} points, {np.mean(counts == len(trip) + 1):.3f} of the tracks "
              f"reach the last frame")
    if dense:                        # likewise; one call for the clip
        dtracks, dstart, dlen, info = b.dense_tracks(da.ptr, w, h, *dense)
        if select is not None:       # the files below hold the kept tracks
            models = b.global_motion(w, h, fb_check=True)[0] if opts["--global-motion"] else None
            try:
                dcode, counts, dtracks, dstart, dlen, _, dindex, _ = capi.track_select(
                    dtracks, dstart, dlen, models, (w, h), capi.TrackSelectParams(**select), shape=False)
            except capi.OfdisError as e:
                sys.exit(f"--track-select: {e}")
            np.save(stem + "_dcode.npy", dcode)
            np.save(stem + "_dindex.npy", dindex)
            print(f"{stem}_dcode.npy, _dindex.npy: of {info[0]} tracks " +
                  ", ".join(f"{c} {name}" for name, c in zip(tracking.TS_NAMES, counts) if c or name == "kept"))
        np.save(stem + "_dtracks.npy", dtracks)
        np.save(stem + "_dstart.npy", dstart)
        np.save(stem + "_dlen.npy", dlen)
        print(f"{stem}_dtracks.npy, _dstart.npy, _dlen.npy: {len(dlen)} tracks ({int((dstart > 0).sum())} seeded after frame 0, "
              f"{info[1]} seeds dropped), mean length {dlen.mean() if len(dlen) else 0:.2f} frames")
    if opts["--reverse"]:            # both directions and both masks in one launch; the forward flow is upsample()'s
        full, rev, mask_fw, mask_rev = b.upsample_bidir(w, h)
        if desc:                     # on the materialised forward flows (include/ofdis.h: no form on the level flows)
            if not 1 <= desc[2] <= dtracks.shape[0] - 1 or not capi.track_descriptor_dims(*desc[:3]):
                sys.exit("--descriptors: N even, 2..64; NXY 1..4, dividing N; NT 1..8 and at most the tracks' Lmax")
            dhist, dshape = capi.track_descriptors(np.stack(frames_a + frames_b), full, dtracks, dstart, dlen, *desc)
            np.save(stem + "_dhist.npy", dhist)
            np.save(stem + "_dshape.npy", dshape)
            print(f"{stem}_dhist.npy, _dshape.npy: {dhist.shape[0]} descriptors of {dhist.shape[1]} entries, largest "
                  f"{int(dhist.max(initial=0))}")
    else:
        full = b.upsample(w, h)      # [pairs][h][w][2] (one channel in stereo mode)
    b.close()
    da.free()
    db.free()
    for t, f in zip(trip, full):
        if opts["--stereo"]:
            write_pfm(t[2], f[..., 0])
        else:
            write_flo(t[2], f)
        mag = np.sqrt((f.astype(np.float64) ** 2).sum(-1))
        print(f"{t[2]}: {w}x{h}, mean |flow| {mag.mean():.3f} px, max {mag.max():.2f}")
    if opts["--reverse"]:
        for k, t in enumerate(trip):
            stem = t[2][:-4] if t[2].endswith(".flo") else t[2]
            write_flo(stem + ".rev.flo", rev[k])
            write_pgm(stem + ".mask.pgm", mask_fw[k])
            write_pgm(stem + ".rev.mask.pgm", mask_rev[k])
            print(f"{stem}.rev.flo, .mask.pgm, .rev.mask.pgm: consistent {np.mean(mask_fw[k] == 0):.3f} / "
                  f"{np.mean(mask_rev[k] == 0):.3f} of the pixels")


if __name__ == "__main__":
    main(sys.argv[1:])
