"""Shared helpers for the test-suite: seeded synthetic inputs (tools/gen_synth.py) and pyramids."""
import functools
import os

import numpy as np

import gen_synth
import oracle
from of_dis_amd.abi import bind, prototypes
from of_dis_amd.params import oppoint

_f32 = np.float32
TESTHOOKS_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "ofdis_test_hooks.h")


def testhook_prototypes():
    """name -> (restype, [argtypes]) of every function tests/csrc/ofdis_test_hooks.h declares, by the parser that binds the
    product, with the few types only the hooks use"""
    return prototypes(open(TESTHOOKS_HEADER).read(), hook_types=True)


@functools.lru_cache(maxsize=None)
def testhooks():
    """The TEST library (tests/csrc/ofdis_testhooks.hip and ofdis_launch_hooks*.hip, built by of_dis_amd.build next to the
    product), opened once, every function with the prototype its header declares.  Not part of the shipped library.  No
    fallback: a library without one of the declared functions is a failure."""
    import ctypes as C
    from of_dis_amd import build
    path = build.testhooks_path()
    if not os.path.exists(path):
        build.build()
    return bind(C.CDLL(path), testhook_prototypes())


def wave_sum_test(gpu, x):
    x = np.ascontiguousarray(x, _f32)
    with gpu.DeviceCall() as c:
        assert testhooks().ofdis_test_wave_sum(c.input(x), c.output(x.shape), x.size, None) == 0
        return c.results()[0]


def div_sqrt_test(gpu, a, b):
    """Rows: div_rn(a,b), a/b, sqrt_rn(|a|), sqrtf(|a|), the fused TV kernel's quotient a/b, its quotient b / sqrt(|a|),
    computed on the device (ofdis_dev.h)."""
    a, b = np.ascontiguousarray(a, _f32), np.ascontiguousarray(b, _f32)
    with gpu.DeviceCall() as c:
        assert testhooks().ofdis_test_div_sqrt(c.input(a), c.input(b), c.output((6, a.size)), a.size, None) == 0
        return c.results()[0]


@functools.lru_cache(maxsize=16)
def synth_case(width, height, seed=1234, channels=1, op_point=2, usetvref=None):
    """Returns (params, pyr_a[img,dx,dy], pyr_b[img,dx,dy], gt_flow, (ia, ib)) for a synthetic pair."""
    ia, ib, gt = gen_synth.make_pair(width, height, seed, channels)
    p = oppoint(op_point, width, height, noc=channels, usetvref=usetvref)
    O = oracle.c_oracle()
    pa = O.build_pyramid(p, ia)
    pb = O.build_pyramid(p, ib)
    return p, pa, pb, gt, (ia, ib)


def rand_planes(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(_f32)


def assert_bits_equal(a, b, what=""):
    a = np.ascontiguousarray(a, dtype=_f32)
    b = np.ascontiguousarray(b, dtype=_f32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    eq = (a == b) | (np.isnan(a) & np.isnan(b))
    if not eq.all():
        bad = np.argwhere(~eq)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {a.size} values differ; first at {i}: {a[i]!r} vs {b[i]!r}; "
                             f"max abs diff {np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))}")
