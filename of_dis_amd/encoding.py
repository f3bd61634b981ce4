"""Numpy model of the output encodings of include/ofdis.h (ofdis_encoding): what ofdis_encode and
ofdis_batch_upsample_frames_enc compute, operation by operation in float32, the decoder a consumer of the encoded arrays
needs, and the named presets.  Needs numpy only (no GPU, no library): the tests compare the kernels against `encode`.

    from of_dis_amd import encoding
    q = batch.upsample_frames_enc(0, n, w, h, encoding.KITTI_FLOW)     # uint16 [n][h][w][2]
    flow = encoding.decode(q, encoding.KITTI_FLOW)                     # float32, within 1/128 px of the fp32 result
"""
import numpy as np

from .capi import ENC_F16, ENC_F32, ENC_U8, ENC_U16, Encoding

_f32 = np.float32
_MAX = {ENC_U16: 65535, ENC_U8: 255}

F32 = Encoding(ENC_F32)
F16 = Encoding(ENC_F16)
# KITTI flow .png: uint16 = 64 * flow + 2^15 per component (the devkit's flow_write)
KITTI_FLOW = Encoding(ENC_U16, 64.0, 32768.0)
# KITTI disparity .png: uint16 = 256 * disparity, disparity >= 0; the left-view result of the stereo-depth mode is <= 0
KITTI_DISPARITY = Encoding(ENC_U16, -256.0, 0.0)


def u8_bound(bound):
    """The two-stream dataset format: flow clipped to [-bound, bound] and mapped linearly onto 0..255 (bound 20 is the
    usual choice)."""
    bound = float(bound)
    if not (bound > 0.0 and np.isfinite(bound)):
        raise ValueError("bound must be positive and finite")
    return Encoding(ENC_U8, _f32(255.0) / _f32(2.0 * bound), 127.5)


def encode(a, enc):
    """The header's arithmetic on a float32 array: returns enc.dtype, same shape."""
    a = np.asarray(a, _f32)
    if enc.type == ENC_F32:
        return a.copy()
    if enc.type == ENC_F16:
        with np.errstate(over="ignore", invalid="ignore"):
            return a.astype(np.float16)  # round to nearest even, gradual underflow, overflow to inf
    m = _f32(_MAX[enc.type])  # (KeyError: an unknown type)
    with np.errstate(over="ignore", invalid="ignore"):
        t = a * _f32(enc.scale) + _f32(enc.offset)  # two float32 roundings
        t = np.fmin(np.fmax(t, _f32(0.0)), m)       # fmaxf / fminf: a NaN becomes 0
        q = np.floor(t + _f32(0.5))
    assert t.dtype == _f32 and q.dtype == _f32
    return q.astype(enc.dtype)


def decode(q, enc):
    """float32 values from an encoded array: exact for F32 and F16, (q - offset) / scale for the integer types."""
    q = np.asarray(q)
    if enc.type in (ENC_F32, ENC_F16):
        return q.astype(_f32)
    return (q.astype(_f32) - _f32(enc.offset)) / _f32(enc.scale)
