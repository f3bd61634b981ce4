"""The sequence driver (of_dis_amd/csrc/host/run_seq_main.cpp) as it is, on the CPU: linked against tests/c/ofdis_abi_stub.c, a
host-only stand-in for the library whose "flow" of a pair is an element-wise function of the pair's two frames (stub_flow
below states it in numpy).  Every file the driver writes is compared, byte for byte, with that function of the input images
in the format the options ask for: a wrong frame, buffer slot, carried frame or stale buffer changes the bytes.  What no GPU
test may provoke is injected by the stub (OFDIS_STUB_FAIL_*): a chunk whose enqueue fails, a pass that reports itself lost and
is repeated, a pinned allocation that fails.  OFDIS_SEQ_STUB_DIR names a directory with other builds of the two programs
(tools/host_sanitize.sh: AddressSanitizer + UBSan, ThreadSanitizer); a sanitizer report changes the exit status and fails
the case.  The failed-pair COUNT of a run is not printed by the driver: the tests pin the set of files and the exit status."""
import os
import struct
import subprocess

import numpy as np
import pytest

from of_dis_amd import encoding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB_DIR = os.environ.get("OFDIS_SEQ_STUB_DIR") or os.path.join(ROOT, "of_dis_amd", "lib")
OF_INT = os.path.join(STUB_DIR, "run_OF_INT_seq_stub")   # gray frames, two flow channels, .flo
DE_RGB = os.path.join(STUB_DIR, "run_DE_RGB_seq_stub")   # colour frames, one displacement channel, .pfm

W, H, NFRAMES = 64, 48, 8
NPAIRS = NFRAMES - 1                                     # pair k = (frame k, frame k + 1), in both kinds of list


def write_pnm(path, img):
    """img: uint8 [h][w] (P5) or [h][w][3] in R, G, B order (P6)"""
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n255\n" % (b"P5" if img.ndim == 2 else b"P6", img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def stub_flow(fa, fb, nch):
    """tests/c/ofdis_abi_stub.c: ofdis_batch_upsample_frames_enc, on frames as the driver holds them ([h][w][noc], colour as
    B, G, R): float32 [h][w][nch]."""
    fa, fb = fa.astype(np.float32), fb.astype(np.float32)
    ch = [np.float32(0.25) * fa[..., 0] - np.float32(0.125) * fb[..., -1],
          np.float32(0.03125) * fb[..., 0] - np.float32(0.5) * fa[..., -1] + np.float32(1.0)]
    return np.stack(ch[:nch], axis=-1)


def flo_bytes(v):
    return b"PIEH" + struct.pack("<ii", v.shape[1], v.shape[0]) + v.astype("<f4").tobytes()


def pfm_bytes(v):  # rows bottom-up, values negated (host/image_io.cpp: write_pfm)
    return b"Pf\n%d %d\n-1.000000\n" % (v.shape[1], v.shape[0]) + (-v[::-1, :, 0]).astype("<f4").tobytes()


def pgm_bytes(q):  # uint8 or uint16 [h][w]; 16-bit samples most significant byte first
    return b"P5\n%d %d\n%d\n" % (q.shape[1], q.shape[0], 255 if q.dtype == np.uint8 else 65535) + q.astype(q.dtype.newbyteorder(">")).tobytes()


LINKS = {"f32": encoding.F32, "f16": encoding.F16, "u8:20": encoding.u8_bound(20), "kitti": encoding.KITTI_FLOW}


def result_files(out, flow, link="f32", stereo=False):
    """{path: bytes} of one pair's result `flow` (float32 [h][w][nch]) written to the list's name `out` over --link `link`"""
    enc = encoding.KITTI_DISPARITY if stereo and link == "kitti" else LINKS[link]
    q = encoding.encode(flow, enc)
    if link in ("f32", "f16"):
        wide = q.astype(np.float32)
        return {out: pfm_bytes(wide) if stereo else flo_bytes(wide)}
    if stereo:
        return {out + ".pgm": pgm_bytes(q[..., 0])}
    return {out + ".u.pgm": pgm_bytes(q[..., 0]), out + ".v.pgm": pgm_bytes(q[..., 1])}


class Clip:
    """NFRAMES frames on disk, once per module and never changed, with three files no pair can use"""

    def __init__(self, root, channels):
        rng = np.random.default_rng(20 + channels)
        shape = (H, W) if channels == 1 else (H, W, 3)
        ext = "pgm" if channels == 1 else "ppm"
        self.frames, self.paths = [], []
        for k in range(NFRAMES):
            img = rng.integers(0, 256, shape, dtype=np.uint8)
            self.paths.append(str(root / f"f{k}.{ext}"))
            write_pnm(self.paths[-1], img)
            self.frames.append(img[..., None] if channels == 1 else img[..., ::-1])  # as read: [h][w][noc], B, G, R
        self.missing = str(root / f"missing.{ext}")
        self.garbage = str(root / f"garbage.{ext}")
        with open(self.garbage, "wb") as f:
            f.write(b"not an image at all\n")
        self.small = str(root / f"small.{ext}")
        write_pnm(self.small, rng.integers(0, 256, (H // 2, W // 2) + shape[2:], dtype=np.uint8))

    def flow(self, k, nch):
        return stub_flow(self.frames[k], self.frames[k + 1], nch)


@pytest.fixture(scope="module")
def gray(tmp_path_factory):
    return Clip(tmp_path_factory.mktemp("gray"), 1)


@pytest.fixture(scope="module")
def colour(tmp_path_factory):
    return Clip(tmp_path_factory.mktemp("colour"), 3)


def run_driver(exe, args, env=None):
    assert os.path.exists(exe), f"{exe} missing: python -m of_dis_amd.build"
    knobs = {k: v for k, v in os.environ.items() if not k.startswith("OFDIS_STUB_")}
    knobs.update(env or {})
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60, env=knobs)


def pairs_list(tmp, clip, ext, bad=None):
    """A pairs list over the clip: (list path, output names).  bad: {(pair, 0 or 1): path} replaces one image of a pair."""
    out = tmp / "out"
    out.mkdir()
    names = [str(out / f"o{k}.{ext}") for k in range(NPAIRS)]
    lines = ["# img1 img2 out\n", "\n"]
    for k in range(NPAIRS):
        a, b = (bad or {}).get((k, 0), clip.paths[k]), (bad or {}).get((k, 1), clip.paths[k + 1])
        lines.append(f"{a} {b} {names[k]}\n")
    (tmp / "pairs.txt").write_text("".join(lines))
    return tmp / "pairs.txt", names


def frames_list(tmp, clip, bad=None):
    """A frame list over the clip: (list path, output names).  bad: {frame: path}."""
    out = tmp / "out"
    out.mkdir()
    names = [str(out / f"o{k}.flo") for k in range(NPAIRS)]
    lines = [f"{(bad or {}).get(k, clip.paths[k])} {names[k] if k < NPAIRS else ''}".rstrip() + "\n" for k in range(NFRAMES)]
    (tmp / "frames.txt").write_text("# img out\n" + "".join(lines))
    return tmp / "frames.txt", names


def check_files(tmp, clip, names, written, link="f32", stereo=False):
    """Exactly the results of the pairs `written` stand in the output directory, each whole and right."""
    expect = {}
    for k in written:
        expect.update(result_files(names[k], clip.flow(k, 1 if stereo else 2), link, stereo))
    assert sorted(os.listdir(tmp / "out")) == sorted(os.path.basename(p) for p in expect)
    for path, data in expect.items():
        with open(path, "rb") as f:
            assert f.read() == data, path


ALL = range(NPAIRS)


# ---------------------------------------------------------------------------------------------- complete runs
@pytest.mark.parametrize("opts", [["--chunk", 3], ["--chunk", 2, "--devices", "0,1", "--depth", 3], ["--chunk", 16]],
                         ids=["short-last-chunk", "two-devices-depth-3", "chunk-larger-than-the-share"])
def test_pairs_list(gray, tmp_path, opts):
    lst, names = pairs_list(tmp_path, gray, "flo")
    r = run_driver(OF_INT, [lst] + opts)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    check_files(tmp_path, gray, names, ALL)
    shares = 2 if "--devices" in opts else 1
    assert sum(l.startswith("TIME (share ") for l in r.stdout.splitlines()) == shares
    assert f"TIME ({NPAIRS} pairs on {shares} device share(s), chunk {opts[1]}," in r.stdout
    if shares == 2:
        assert "TIME (share 1: device 1 [0000:01:00.0], pairs 4..6," in r.stdout


@pytest.mark.parametrize("opts", [["--chunk", 2, "--devices", "0,0"], ["--chunk", 1, "--depth", 1]],
                         ids=["a-frame-decoded-by-both-shares", "every-chunk-carries-its-frame-over"])
def test_frame_list_gives_the_files_of_the_pairs_list(gray, tmp_path, opts):
    lst, names = frames_list(tmp_path, gray)
    r = run_driver(OF_INT, [lst, "--sequence", 1] + opts)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    check_files(tmp_path, gray, names, ALL)


@pytest.mark.parametrize("link", ["f16", "u8:20", "kitti"])
def test_link_encodings(gray, tmp_path, link):
    lst, names = pairs_list(tmp_path, gray, "flo")
    r = run_driver(OF_INT, [lst, "--chunk", 3, "--link", link])
    assert r.returncode == 0 and r.stderr == "", r.stderr
    check_files(tmp_path, gray, names, ALL, link)


def test_stereo_program(colour, tmp_path):
    """run_DE_*_seq: one channel, .pfm (--link kitti: the disparity encoding, one .pgm); a list of stereo pairs is no sequence"""
    lst, names = pairs_list(tmp_path, colour, "pfm")
    r = run_driver(DE_RGB, [lst, "--chunk", 3])
    assert r.returncode == 0 and r.stderr == "", r.stderr
    check_files(tmp_path, colour, names, ALL, stereo=True)
    for n in names:
        os.remove(n)
    r = run_driver(DE_RGB, [lst, "--chunk", 3, "--link", "kitti"])
    assert r.returncode == 0 and r.stderr == "", r.stderr
    check_files(tmp_path, colour, names, ALL, "kitti", stereo=True)
    for n in names:
        os.remove(n + ".pgm")
    r = run_driver(DE_RGB, [lst, "--sequence", 1])
    assert r.returncode == 2 and "--sequence: a list of stereo pairs is not a sequence" in r.stderr
    assert os.listdir(tmp_path / "out") == []


# ---------------------------------------------------------------------------------------------- images no pair can use
def test_pairs_list_with_unusable_images(gray, tmp_path):
    """--chunk 3 = pairs 0..2 | 3..5 | 6: the first image of the first pair (the geometry then comes from pair 1), the first
    image of a chunk and an image in the middle of a chunk.  One stderr line per failed pair, the other pairs right."""
    bad = {(0, 0): gray.missing, (3, 0): gray.small, (4, 1): gray.garbage}
    lst, names = pairs_list(tmp_path, gray, "flo", bad)
    r = run_driver(OF_INT, [lst, "--chunk", 3])
    assert r.returncode == 1
    lines = r.stderr.splitlines()
    assert len(lines) == 3, r.stderr
    assert sum(gray.missing in l for l in lines) == 1 and sum(gray.garbage in l for l in lines) == 1
    assert f"{gray.small} / {gray.paths[4]}: not {W}x{H} like the first readable pair" in lines
    check_files(tmp_path, gray, names, [1, 2, 5, 6])


def test_frame_list_with_unusable_frames(gray, tmp_path):
    """--chunk 2 = frames 0..2 | 2..4 | 4..6 | 6..7: frame 2 is the one chunk 1 takes over from chunk 0, frame 5 stands in the
    middle of its chunk.  Each costs the two pairs it belongs to and is named once."""
    lst, names = frames_list(tmp_path, gray, {2: gray.missing, 5: gray.small})
    r = run_driver(OF_INT, [lst, "--sequence", 1, "--chunk", 2])
    assert r.returncode == 1
    lines = r.stderr.splitlines()
    assert len(lines) == 2, r.stderr
    assert sum(gray.missing in l for l in lines) == 1
    assert f"{gray.small}: not {W}x{H} like the first readable frame" in lines
    check_files(tmp_path, gray, names, [0, 3, 6])


@pytest.mark.parametrize("sequence", [False, True], ids=["pairs", "frames"])
def test_buffer_slots_that_were_never_written(gray, tmp_path, sequence):
    """--chunk 2 --depth 1: four chunks rotate through three buffers.  Pair 0 (frame 0) is unreadable, so slot 0 of the first
    buffer goes to the device without ever having held an image, and the short last chunk (pair 6 alone) takes over the
    buffer that held the two pairs of the first chunk."""
    if sequence:
        lst, names = frames_list(tmp_path, gray, {0: gray.garbage})
    else:
        lst, names = pairs_list(tmp_path, gray, "flo", {(0, 0): gray.garbage})
    r = run_driver(OF_INT, [lst, "--chunk", 2, "--depth", 1, "--size", W, H] + (["--sequence", 1] if sequence else []))
    assert r.returncode == 1
    assert len(r.stderr.splitlines()) == 1 and gray.garbage in r.stderr
    check_files(tmp_path, gray, names, range(1, NPAIRS))


# ---------------------------------------------------------------------------------------------- injected failures
# one share, --chunk 2 = pairs 0,1 | 2,3 | 4,5 | 6
@pytest.mark.parametrize("depth", [1, 2])
def test_a_chunk_whose_enqueue_fails(gray, tmp_path, depth):
    """The third ofdis_batch_run fails: the two chunks enqueued before it are written, whole; nothing of the third and fourth"""
    lst, names = pairs_list(tmp_path, gray, "flo")
    r = run_driver(OF_INT, [lst, "--chunk", 2, "--depth", depth], {"OFDIS_STUB_FAIL_RUN": "3"})
    assert r.returncode == 1
    assert r.stderr.splitlines() == ["share 0 (device 0, pairs 0..6): chunk: stub: injected failure of ofdis_batch_run"]
    check_files(tmp_path, gray, names, range(4))


@pytest.mark.parametrize("depth", [1, 2])
def test_a_lost_pass_is_repeated_once(gray, tmp_path, depth):
    lst, names = pairs_list(tmp_path, gray, "flo")
    r = run_driver(OF_INT, [lst, "--chunk", 2, "--depth", depth], {"OFDIS_STUB_FAIL_STATUS": "2"})
    assert r.returncode == 0
    assert r.stderr.splitlines() == ["stub: injected lost pass"]
    check_files(tmp_path, gray, names, ALL)


@pytest.mark.parametrize("depth", [1, 2])
def test_a_pinned_allocation_that_fails(gray, tmp_path, depth):
    """A chunk buffer of a pairs list is three pinned allocations, made when the buffer is first used: the 8th belongs to the
    third chunk."""
    lst, names = pairs_list(tmp_path, gray, "flo")
    r = run_driver(OF_INT, [lst, "--chunk", 2, "--depth", depth], {"OFDIS_STUB_FAIL_HOST_ALLOC": "8"})
    assert r.returncode == 1
    assert r.stderr.splitlines() == ["ofdis_host_alloc: stub: injected failure of ofdis_host_alloc",
                                     "share 0 (device 0, pairs 0..6): pinned host memory"]
    check_files(tmp_path, gray, names, range(4))


def test_device_bench_counts_chunks_and_writes_nothing(gray, tmp_path):
    """6 passes of the first chunk at depth 2: the first depth + 2 fill the buffers and are not counted"""
    lst, _ = pairs_list(tmp_path, gray, "flo")
    r = run_driver(OF_INT, [lst, "--device-bench", 6, "--chunk", 2])
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert "DEVICE STAGE (share 0: 2 chunks of 2 pairs, 2 in flight): " in r.stdout
    assert os.listdir(tmp_path / "out") == []


# ---------------------------------------------------------------------------------------------- option errors
@pytest.mark.parametrize("opts,status,message", [
    (["--bogus", 1], 2, "unknown option --bogus"),
    (["--chunk"], 2, "--chunk needs a value"),
    (["--size", 64], 2, "--size needs W H"),
    (["--link", "u8:0"], 2, "--link u8:0: not a link format"),
    (["--chunk", 0], 2, "--chunk must be 1..65535"),
    (["--chunk", 65536], 2, "--chunk must be 1..65535"),
    (["--depth", 0], 2, "--depth must be 1..8"),
    (["--depth", 9], 2, "--depth must be 1..8"),
    (["--devices", "0,2"], 1, "device 2 requested, 2 HIP device(s) visible"),
], ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else None)
def test_option_errors_end_the_program_before_any_device_call(gray, tmp_path, opts, status, message):
    lst, _ = pairs_list(tmp_path, gray, "flo")
    # (a device call after the message would be this run's first ofdis_batch_run, and would add its own line)
    r = run_driver(OF_INT, [lst] + opts, {"OFDIS_STUB_FAIL_RUN": "1"})
    assert r.returncode == status
    assert r.stderr.splitlines()[0] == message and (len(r.stderr.splitlines()) == 1 or opts[0] == "--link"), r.stderr
    assert r.stdout == "" and os.listdir(tmp_path / "out") == []
