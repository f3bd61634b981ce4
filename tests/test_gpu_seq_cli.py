"""run_OF_INT_seq --sequence 1: a list of FRAMES ("img out.flo" per frame, the last line "img" alone) through sequence
contexts -- every frame decoded, uploaded and built once, the frame two chunks share carried over on the host -- writes the
files the pairs list of the same pairs writes."""
import os
import subprocess

import pytest

import gen_synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "of_dis_amd", "lib", "run_OF_INT_seq")
W, H, NFRAMES = 256, 112, 5


def _lists(tmp_path, tag_seq, tag_pairs, ext):
    """five frames of one moving scene on disk; the frame list and the pairs list of the same four pairs"""
    names = []
    for k in range(NFRAMES):
        ia, ib, _ = gen_synth.make_pair(W, H, 900, flow_scale=0.5 * k)
        names.append(str(tmp_path / f"f{k}.pgm"))
        if not os.path.exists(names[-1]):
            gen_synth.write_pgm(names[-1], ib if k else ia)
    seq, pairs = tmp_path / f"{tag_seq}.txt", tmp_path / f"{tag_pairs}.txt"
    seq.write_text("# a clip\n" + "".join(f"{names[k]} {tmp_path}/{tag_seq}{k}.{ext}\n" for k in range(NFRAMES - 1)) + names[-1] + "\n")
    pairs.write_text("".join(f"{names[k]} {names[k + 1]} {tmp_path}/{tag_pairs}{k}.{ext}\n" for k in range(NFRAMES - 1)))
    return seq, pairs


def test_sequence_list_dry_run_prints_the_pairs_partition(tmp_path):
    seq, pairs = _lists(tmp_path, "s", "p", "flo")
    a = subprocess.run([EXE, str(seq), "--sequence", "1", "--chunk", "2", "--devices", "0,0", "--dry-run", "1"], capture_output=True, text=True)
    b = subprocess.run([EXE, str(pairs), "--chunk", "2", "--devices", "0,0", "--dry-run", "1"], capture_output=True, text=True)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout == "share 0: device 0 pairs 0..1\nshare 1: device 0 pairs 2..3\n"


@pytest.mark.gpu
@pytest.mark.parametrize("link,suffixes", [(None, [""]), ("u8:20", [".u.pgm", ".v.pgm"])], ids=["f32", "u8-bound-20"])
def test_sequence_list_writes_the_files_of_the_pairs_list(gpu, tmp_path, link, suffixes):
    """--chunk 2 --devices 0,0 over four pairs: two shares of two pairs, so frame 2 ends one share and starts the next (decoded
    by both), and with --chunk 1 every share carries its middle frame from one chunk to the next."""
    opts = ["--link", link] if link else []
    seq, pairs = _lists(tmp_path, "s", "p", "flo")
    r = subprocess.run([EXE, str(pairs), "--chunk", "2", "--devices", "0,0"] + opts + ["2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    want = [open(f"{tmp_path}/p{k}.flo{s}", "rb").read() for k in range(NFRAMES - 1) for s in suffixes]
    assert len(set(want)) == len(want)
    for chunk, devices in (("2", "0,0"), ("1", "0,0"), ("3", "0"), ("1", "0")):
        r = subprocess.run([EXE, str(seq), "--sequence", "1", "--chunk", chunk, "--devices", devices] + opts + ["2"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        got = []
        for k in range(NFRAMES - 1):
            for s in suffixes:
                path = f"{tmp_path}/s{k}.flo{s}"
                got.append(open(path, "rb").read())
                os.remove(path)
        assert got == want, f"--chunk {chunk} --devices {devices}: " + str([a == b for a, b in zip(got, want)])


@pytest.mark.gpu
def test_sequence_list_with_an_unreadable_frame(gpu, tmp_path):
    """a missing frame costs the two pairs it belongs to, whichever chunk or share they fall into; the others are written"""
    seq, pairs = _lists(tmp_path, "s", "p", "flo")
    r = subprocess.run([EXE, str(pairs), "--chunk", "2", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    os.remove(tmp_path / "f2.pgm")
    r = subprocess.run([EXE, str(seq), "--sequence", "1", "--chunk", "2", "--size", str(W), str(H), "2"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "f2.pgm" in r.stderr, (r.returncode, r.stderr)
    for k in (0, 3):
        assert open(f"{tmp_path}/s{k}.flo", "rb").read() == open(f"{tmp_path}/p{k}.flo", "rb").read()
    for k in (1, 2):
        assert not os.path.exists(f"{tmp_path}/s{k}.flo")
