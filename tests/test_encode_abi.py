"""CPU: the output encodings (include/ofdis.h: ofdis_encoding) -- element sizes, the argument checks of ofdis_encode that
return before any device work (host buffers stand in for the device arrays: every call here returns before it would launch),
the numpy model of the arithmetic (of_dis_amd/encoding.py) on hand-computed values, and the --link option of the sequence
drivers.  The kernels against the model, and the checks that need a context: tests/test_gpu_encode.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import abi
from of_dis_amd import capi, encoding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "of_dis_amd", "lib")
SEQ = {"flow": os.path.join(LIB, "run_OF_INT_seq"), "stereo": os.path.join(LIB, "run_DE_INT_seq")}
_f32 = np.float32


def test_constants_match_the_header():
    types = tuple(abi.enumerator("OFDIS_ENC_" + n) for n in ("F32", "F16", "U16", "U8"))
    assert types == (capi.ENC_F32, capi.ENC_F16, capi.ENC_U16, capi.ENC_U8)
    assert abi.define("OFDIS_VERSION") == 3  # no struct layout changed
    assert C.sizeof(capi.Encoding) == 12


def test_encoding_bytes():
    L = capi.lib()
    assert [L.ofdis_encoding_bytes(t) for t in (capi.ENC_F32, capi.ENC_F16, capi.ENC_U16, capi.ENC_U8)] == [4, 2, 2, 1]
    for t in (-1, 4, 17, 1 << 20):
        assert L.ofdis_encoding_bytes(t) == 0
    for enc in (encoding.F32, encoding.F16, encoding.KITTI_FLOW, encoding.u8_bound(20)):
        assert enc.dtype.itemsize == L.ofdis_encoding_bytes(enc.type)


# ------------------------------------------------------------------ ofdis_encode: argument errors before any device work
def _encode(enc, src=True, dst=True, same=False, n=8):
    a = np.zeros(16, _f32)
    o = np.zeros(16, _f32)
    sp = a.ctypes.data if src else None
    dp = (a.ctypes.data if same else o.ctypes.data) if dst else None
    return capi.lib().ofdis_encode(sp, dp, n, C.byref(enc) if enc is not None else None, None)


@pytest.mark.parametrize("which", ["src", "dst"])
def test_encode_rejects_null_pointers(which):
    abi.rejected(_encode(encoding.F16, **{which: False}))


def test_encode_rejects_a_null_encoding():
    abi.rejected(_encode(None))


@pytest.mark.parametrize("t", [-1, 4, 100])
def test_encode_rejects_an_unknown_type(t):
    abi.rejected(_encode(capi.Encoding(t, 1.0, 0.0)))
    assert "type" in capi.lib().ofdis_last_error().decode()


@pytest.mark.parametrize("t", [capi.ENC_U16, capi.ENC_U8])
@pytest.mark.parametrize("scale", [0.0, -0.0, math.inf, -math.inf, math.nan])
def test_encode_rejects_a_bad_scale(t, scale):
    abi.rejected(_encode(capi.Encoding(t, scale, 0.0)))
    assert "scale" in capi.lib().ofdis_last_error().decode()


@pytest.mark.parametrize("t", [capi.ENC_U16, capi.ENC_U8])
@pytest.mark.parametrize("offset", [math.inf, -math.inf, math.nan])
def test_encode_rejects_a_bad_offset(t, offset):
    abi.rejected(_encode(capi.Encoding(t, 1.0, offset)))
    assert "offset" in capi.lib().ofdis_last_error().decode()


@pytest.mark.parametrize("enc", [encoding.F32, encoding.F16, encoding.KITTI_FLOW, encoding.u8_bound(20)], ids=repr)
def test_encode_rejects_in_place(enc):
    abi.rejected(_encode(enc, same=True))


def test_upsample_frames_enc_without_a_context():
    out = np.zeros(16, _f32)
    abi.rejected(capi.lib().ofdis_batch_upsample_frames_enc(None, 0, 1, out.ctypes.data, 8, 4, C.byref(encoding.F16), None))


# ------------------------------------------------------------------ the numpy model
def test_presets():
    k = encoding.KITTI_FLOW
    assert (k.type, k.scale, k.offset) == (capi.ENC_U16, 64.0, 32768.0)
    d = encoding.KITTI_DISPARITY
    assert (d.type, d.scale, d.offset) == (capi.ENC_U16, -256.0, 0.0)
    b = encoding.u8_bound(20)
    assert (b.type, b.scale, b.offset) == (capi.ENC_U8, 6.375, 127.5)  # 255 / 40
    for bad in (0, -1, math.inf, math.nan):
        with pytest.raises(ValueError):
            encoding.u8_bound(bad)


def test_model_kitti_flow_hand_computed():
    v = np.array([0.0, 1.0, -1.0, 0.5, 1.0 / 128, -1.0 / 128, 3.0 / 256, 511.984375, 512.0, -512.0, -513.0, 1e9, -1e9], _f32)
    #             32768  +64  -64   +32  x.5 up     x.5 up       .75 up    65535 exactly  clamp  0      clamp
    want = [32768, 32832, 32704, 32800, 32769, 32768, 32769, 65535, 65535, 0, 0, 65535, 0]
    q = encoding.encode(v, encoding.KITTI_FLOW)
    assert q.dtype == np.uint16 and q.tolist() == want


def test_model_kitti_disparity_hand_computed():
    v = np.array([0.0, -1.0, -0.001953125, -0.005859375, -255.998046875, -256.0, -300.0, 5.0], _f32)
    #             0    256   0.5 -> 1      1.5 -> 2      65535.5 clamps      clamp   clamp   negative side clamps to 0
    want = [0, 256, 1, 2, 65535, 65535, 65535, 0]
    assert encoding.encode(v, encoding.KITTI_DISPARITY).tolist() == want


def test_model_u8_bound_hand_computed():
    v = np.array([0.0, 20.0, -20.0, 25.0, -25.0, 4.0, -4.0, 0.07843137], _f32)
    #             127.5 -> 128 (tie up), 255, 0, clamp, clamp, 153, 102, 20/255 -> 128 +- one ulp, rounds to 128 either way
    want = [128, 255, 0, 255, 0, 153, 102, 128]
    q = encoding.encode(v, encoding.u8_bound(20))
    assert q.dtype == np.uint8 and q.tolist() == want


@pytest.mark.parametrize("enc", [capi.Encoding(capi.ENC_U16, 1.0, 0.0), capi.Encoding(capi.ENC_U8, 1.0, 0.0)], ids=repr)
def test_model_ties_round_up_and_values_clamp(enc):
    m = 65535 if enc.type == capi.ENC_U16 else 255
    v = np.array([0.5, 1.5, 2.5, 3.5, m - 0.5, -0.5, -1e-3, 0.49999997, m + 0.25, m + 1000, -5, math.inf, -math.inf], _f32)
    # (0.49999997 = 0.5 - 2^-25: the fp32 sum with 0.5 is the tie between 1 - 2^-24 and 1 and rounds to 1, so q = 1 -- the
    # separately rounded addition is part of the definition)
    want = [1, 2, 3, 4, m, 0, 0, 1, m, m, 0, m, 0]
    assert encoding.encode(v, enc).tolist() == want


@pytest.mark.parametrize("enc", [encoding.KITTI_FLOW, encoding.KITTI_DISPARITY, encoding.u8_bound(20)], ids=repr)
def test_model_nan_becomes_zero(enc):
    assert encoding.encode(np.array([math.nan, -math.nan], _f32), enc).tolist() == [0, 0]


def test_model_f16_and_f32():
    v = np.array([1.0, 65504.0, 65519.99, 65520.0, -1e6, 6e-8, 2.98e-8, 1e-10, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], _f32)
    h = encoding.encode(v, encoding.F16)
    assert h.dtype == np.float16
    # overflow from 65520 on; the smallest subnormal half is 2^-24 = 5.96e-8: 6e-8 keeps it, half of it ties to even (0)
    assert h.view(np.uint16).tolist() == [0x3c00, 0x7bff, 0x7bff, 0x7c00, 0xfc00, 0x0001, 0x0000, 0x0000, 0x3c00, 0x3c02]
    assert np.isnan(encoding.encode(np.array([math.nan], _f32), encoding.F16)).all()
    same = encoding.encode(v, encoding.F32)
    assert same.dtype == _f32 and same.view(np.uint32).tolist() == v.view(np.uint32).tolist()


def test_model_decode_inverts_within_half_a_step():
    rng = np.random.default_rng(5)
    v = np.clip(rng.standard_normal(4096) * 6, -19.9, 19.9).astype(_f32)  # inside both ranges: nothing clamps
    for enc, step in ((encoding.KITTI_FLOW, 1 / 64), (encoding.u8_bound(20), 40 / 255)):
        back = encoding.decode(encoding.encode(v, enc), enc)
        # half a quantisation step, plus the rounding of t (at most 2^-9 at t < 65536, i.e. 2^-9 / scale in v) and of the
        # decoder's two operations
        assert back.dtype == _f32 and np.abs(back - v).max() <= step / 2 + 2.0 ** -9 / abs(enc.scale) + 1e-5
    assert np.array_equal(encoding.decode(encoding.encode(v, encoding.F32), encoding.F32), v)
    assert np.array_equal(encoding.decode(encoding.encode(v, encoding.F16), encoding.F16), v.astype(np.float16).astype(_f32))


# ------------------------------------------------------------------ the sequence drivers' --link
def _list(tmp_path):
    lst = tmp_path / "pairs.txt"
    lst.write_text("".join(f"a{i}.pgm b{i}.pgm o{i}.flo\n" for i in range(5)))
    return str(lst)


VALID_LINKS = ["f32", "f16", "u8:20", "u8:0.5", "u16:64:32768", "u16:-256:0", "u16:1e2:-3.5", "kitti"]
BAD_LINKS = ["", "f64", "F16", "u8", "u8:", "u8:0", "u8:-3", "u8:abc", "u8:20x", "u8:inf", "u8:nan", "u16:64", "u16:64:",
             "u16::5", "u16:0:5", "u16:inf:0", "u16:1:nan", "u16:1:2:3", "kitti:2", "u32:1:0"]


@pytest.mark.parametrize("exe", sorted(SEQ))
@pytest.mark.parametrize("link", VALID_LINKS)
def test_driver_accepts_every_valid_link(tmp_path, exe, link):
    r = subprocess.run([SEQ[exe], _list(tmp_path), "--gpus", "2", "--link", link, "--dry-run", "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["share 0: device 0 pairs 0..2", "share 1: device 1 pairs 3..4"]


@pytest.mark.parametrize("link", BAD_LINKS)
def test_driver_rejects_a_malformed_link_with_its_usage(tmp_path, link):
    r = subprocess.run([SEQ["flow"], _list(tmp_path), "--link", link, "--dry-run", "1"], capture_output=True, text=True)
    assert r.returncode == 2, (r.stdout, r.stderr)
    assert "usage" in r.stderr and "--link" in r.stderr and r.stdout == ""
