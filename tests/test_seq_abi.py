"""CPU: argument checks of the video-sequence entry points that return before any device work (include/ofdis.h:
OFDIS_BATCH_SEQUENCE).  The computations themselves: tests/test_gpu_seq.py."""
import ctypes as C
import os
import subprocess

import abi
from of_dis_amd import capi
from of_dis_amd.params import oppoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_value_matches_the_header():
    assert abi.define("OFDIS_BATCH_SEQUENCE") == capi.BATCH_SEQUENCE == 16
    assert capi.BATCH_SEQUENCE & (capi.BATCH_REVERSE | capi.BATCH_STEREO_LR) == 0


def test_create_ex_rejects_stereo_sequences_and_too_many_pairs():
    L = capi.lib()
    p = oppoint(2, 256, 112)
    stereo = p.copy(selectmode=2)
    h = C.c_void_p()
    for params, flags in ((stereo, capi.BATCH_SEQUENCE | capi.BATCH_STEREO_LR), (p, capi.BATCH_SEQUENCE | capi.BATCH_STEREO_LR),
                          (stereo, capi.BATCH_SEQUENCE)):
        assert L.ofdis_batch_create_ex(C.byref(h), C.byref(params), 2, flags) == -1  # INVALID
        assert not h.value
    assert "sequence" in L.ofdis_last_error().decode().lower()
    # (stereo depth with OFDIS_BATCH_REVERSE stays UNSUPPORTED whatever other bits are set)
    assert L.ofdis_batch_create_ex(C.byref(h), C.byref(stereo), 2, capi.BATCH_SEQUENCE | capi.BATCH_REVERSE) == -2
    # nframes + 1 frames ride in grid.y of the plane kernel: refused before anything is allocated
    for flags in (capi.BATCH_SEQUENCE, capi.BATCH_SEQUENCE | capi.BATCH_REVERSE):
        assert L.ofdis_batch_create_ex(C.byref(h), C.byref(p), 65535, flags) == -2  # UNSUPPORTED
        assert not h.value
    assert "65534" in L.ofdis_last_error().decode()
    assert L.ofdis_batch_create_ex(C.byref(h), C.byref(p.copy(width=1001)), 2, capi.BATCH_SEQUENCE) == -1  # bad params first
    assert L.ofdis_batch_create_ex(C.byref(h), C.byref(p), 2, capi.BATCH_SEQUENCE | 8) == -1       # unknown bits stay unknown
    assert L.ofdis_batch_create_ex(C.byref(h), C.byref(p), 2, capi.BATCH_SEQUENCE | 32) == -1


def test_sequence_calls_without_a_context():
    L = capi.lib()
    assert L.ofdis_batch_input_frames(None) == 0
    assert L.ofdis_batch_device_bytes(None) == 0
    assert L.ofdis_batch_upload_frame(None, 0, None, None, None, None) == -1
    assert L.ofdis_batch_build_pyramids_u8_seq(None, None, 0, 0, 16, 16, None) == -1
    assert "OFDIS_BATCH_SEQUENCE" in L.ofdis_last_error().decode()


def test_new_symbols_are_declared_bound_and_exported():
    new = {"ofdis_batch_input_frames", "ofdis_batch_upload_frame", "ofdis_batch_build_pyramids_u8_seq", "ofdis_batch_device_bytes"}
    assert new <= set(capi.ABI_SYMBOLS) and new <= set(abi.exported())


def test_stereo_drivers_reject_sequence_lists(tmp_path):
    """run_DE_*_seq --sequence 1: refused before the list is read"""
    lst = tmp_path / "frames.txt"
    lst.write_text("a.pgm a.pfm\nb.pgm\n")
    for exe in ("run_DE_INT_seq", "run_DE_RGB_seq"):
        r = subprocess.run([os.path.join(ROOT, "of_dis_amd", "lib", exe), str(lst), "--sequence", "1", "--dry-run", "1"],
                           capture_output=True, text=True)
        assert r.returncode == 2 and "--sequence" in r.stderr, (exe, r.returncode, r.stderr)


def test_sequence_list_dry_run_partition(tmp_path):
    """N + 1 frame lines are N pairs: the partition of the pairs list of N lines; malformed sequence lists are refused"""
    exe = os.path.join(ROOT, "of_dis_amd", "lib", "run_OF_INT_seq")
    seq, pairs = tmp_path / "frames.txt", tmp_path / "pairs.txt"
    seq.write_text("".join(f"f{k}.pgm o{k}.flo\n" for k in range(4)) + "# the last frame\nf4.pgm\n")
    pairs.write_text("".join(f"f{k}.pgm f{k + 1}.pgm o{k}.flo\n" for k in range(4)))
    a = subprocess.run([exe, str(seq), "--sequence", "1", "--devices", "0,0,0", "--dry-run", "1"], capture_output=True, text=True)
    b = subprocess.run([exe, str(pairs), "--devices", "0,0,0", "--dry-run", "1"], capture_output=True, text=True)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout and "pairs 0..1" in a.stdout
    for text in ("f0.pgm o0.flo\nf1.pgm o1.flo\n", "f0.pgm o0.flo\nf1.pgm\nf2.pgm\n"):
        seq.write_text(text)
        r = subprocess.run([exe, str(seq), "--sequence", "1", "--dry-run", "1"], capture_output=True, text=True)
        assert r.returncode == 2 and "--sequence" in r.stderr, (text, r.returncode, r.stderr)
