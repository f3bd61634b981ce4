"""ctypes binding of the C ABI (include/ofdis.h) -- the only way Python reaches the product.

There is no CPU fallback: `lib()` raises if of_dis_amd/lib/libofdis_hip.so is missing, and every
call raises OfdisError on a non-zero status.  numpy helpers move data through the library's own
device-memory helpers so that the tests need nothing but the shared library; the benchmark passes
torch device pointers straight through.
"""
import ctypes as C
import os

import numpy as np

from .abi import bind, prototypes
from .params import OfdisParams  # noqa: F401  (the struct callers pass by reference; stays a name of this module)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libofdis_hip.so")
LIB_PATH = os.environ.get("OFDIS_LIB", LIB_PATH)  # developer A/B builds (tools/ab_build.py); the product path is the default
_f32 = np.float32
FP = C.POINTER(C.c_float)
VP = C.c_void_p

K_WARP, K_DERIV, K_SYSTEM, K_SOR, K_PATCH, K_DENSIFY, K_UPDATE, K_FUSED, K_COUNT = range(9)
K_NAMES = ["warp", "derivatives", "tv_system", "sor", "patch_optimize", "densify", "tv_finish", "tv_fused"]

# every constant of include/ofdis.h under its name without the OFDIS_ prefix (checked by tests/test_abi.py)
OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_DEVICE, ERR_NOMEM = 0, -1, -2, -3, -4  # OFDIS_OK / OFDIS_ERR_*
BATCH_REVERSE = 1  # include/ofdis.h: OFDIS_BATCH_REVERSE
BATCH_STEREO_LR = 2  # OFDIS_BATCH_STEREO_LR
BATCH_SEQUENCE = 16  # OFDIS_BATCH_SEQUENCE
FILL_NONE, FILL_INVALIDATE, FILL_BACKGROUND = 0, 1, 2  # OFDIS_FILL_*
LR_FUSED_MAX_WIDTH = 4096  # OFDIS_LR_FUSED_MAX_WIDTH
FB_ALPHA, FB_BETA = 0.01, 0.5  # OFDIS_FB_ALPHA / OFDIS_FB_BETA
FB_CONSISTENT, FB_INCONSISTENT, FB_OUTSIDE = 0, 1, 2
INTERP_MAX_TIMES = 16  # OFDIS_INTERP_MAX_TIMES
ENC_F32, ENC_F16, ENC_U16, ENC_U8 = 0, 1, 2, 3  # OFDIS_ENC_*
TRACK_MAX_POINTS = 1 << 24  # OFDIS_TRACK_MAX_POINTS
DT_MAX_TRACKS, DT_MAX_STRIDE, DT_MAX_WINDOW = 1 << 24, 64, 7  # OFDIS_DT_MAX_*
TS_KEPT, TS_SHORT, TS_INVALID, TS_STATIC, TS_ERRATIC, TS_JUMP, TS_CAMERA = range(7)  # OFDIS_TS_*
TS_ALL_TESTS = 0x3F  # OFDIS_TS_ALL_TESTS
TRACK_SELECT_LANES = 256  # csrc/ofdis_track_select.hip: kTsLanes, the slots of a workgroup and the records of a trip of its scan
DESC_MAX_PATCH = 64  # OFDIS_DESC_MAX_PATCH
BOF_SCALE, BOF_MAX_WORDS = 510, 16384  # OFDIS_BOF_*
KMEANS_MAX_ITERS = 1000  # OFDIS_KMEANS_MAX_ITERS
TRAJ_MAX_RADIUS = 8  # OFDIS_TRAJ_MAX_RADIUS
GM_MAX_SIDE, GM_MAX_FLOW, GM_MAX_ROUNDS = 8192, 4096.0, 8  # OFDIS_GM_MAX_*
GM_TRANSLATION_ONLY, GM_AFFINE = 0, 1  # OFDIS_GM_* model
GM_OK_AFFINE, GM_TRANSLATION, GM_EMPTY = 0, 1, 2  # OFDIS_GM_* status
GM_INLIER, GM_OUTLIER, GM_INVALID = 0, 1, 2  # OFDIS_GM_* label
STAB_MAX_RADIUS, STAB_MIN_DET, STAB_MAX_DET, STAB_MAX_ZOOM = 64, 0.25, 4.0, 16.0  # OFDIS_STAB_*
STAB_MIN_DENOM = 0.5  # include/ofdis.h, "Projective video stabilisation": the denominator bound of usable (no macro there)
BORDER_CONSTANT, BORDER_REPLICATE = 0, 1  # OFDIS_BORDER_*
# include/ofdis.h, "Segments": the limits that section states in prose (no macro there); of_dis_amd/segments.py has the same
SEG_MAX_SEGMENTS, SEG_RECORD_FIELDS, SEG_INFO_FIELDS = 1 << 24, 12, 4
SEG_MOVING = 1 << GM_OUTLIER  # `codes` of the moving objects in a compensate call's labels
# include/ofdis.h, "Object tracks": likewise in prose there; of_dis_amd/segments.py has the same
SEGTRACK_MAX_SEGMENTS, SEGTRACK_MAX_MAPS, SEGTRACK_MAX_TRACKS = 1024, 65536, 1 << 24
SEGTRACK_FIELDS, SEGTRACK_INFO_FIELDS, SEGTRACK_LDS_MAX_SEGMENTS = 12, 4, 128
# csrc/ofdis_segment_tracks.hip: kStGridBlocks, the most workgroups (of four 64-pixel chunks each) of its per-pixel launches: 8
# for each of 256 compute units; kStLdsGridBlocks and kStBandRows, the same for the LDS route of the overlap (max_segments <=
# SEGTRACK_LDS_MAX_SEGMENTS), where a workgroup takes a band of rows of one pair at a time
SEGTRACK_GRID_BLOCKS, SEGTRACK_LDS_GRID_BLOCKS, SEGTRACK_BAND_ROWS = 256 * 8, 256 * 2, 32
OFDIS_VERSION = 3  # include/ofdis.h: the struct layouts below (OfdisTuning: 21 ints) belong to this ABI version


class OfdisTuning(C.Structure):
    """include/ofdis.h: ofdis_tuning -- kernel-selection knobs, every setting bit-identical except `contract`
    (0 = exact arithmetic, 1 = the FMA / fast-reciprocal tolerance contract)."""
    _fields_ = [(n, C.c_int) for n in ("gray8", "rgb12", "rgb12_lpp", "fused_tv", "fused_mw_max", "fused_split",
                                       "finish_fusion", "fused_strip", "prep_band_rows", "graph", "flow_dma", "flow_whole",
                                       "fused_xcu_max", "fused_tp_pipe", "fused_xcu_spin", "contract", "fused_xcu_drop", "prep_densify", "fused_tall_group", "fused_rgb_min",
                                       "patch_window_reuse")]


class Encoding(C.Structure):
    """include/ofdis.h: ofdis_encoding -- an output format of the full-resolution result.  of_dis_amd/encoding.py has the
    numpy model of its arithmetic, the presets and the decoder."""
    _fields_ = [("type", C.c_int), ("scale", C.c_float), ("offset", C.c_float)]

    def __init__(self, type=ENC_F32, scale=1.0, offset=0.0):
        super().__init__(int(type), float(scale), float(offset))

    @property
    def dtype(self):
        """numpy dtype of one encoded element"""
        return np.dtype({ENC_F32: np.float32, ENC_F16: np.float16, ENC_U16: np.uint16, ENC_U8: np.uint8}[self.type])

    def __repr__(self):
        return f"Encoding(type={self.type}, scale={self.scale!r}, offset={self.offset!r})"


class TrackSelectParams(C.Structure):
    """include/ofdis.h: ofdis_track_select_params.  TrackSelectParams() holds the defaults (ofdis_track_select_defaults);
    keywords replace single values.  of_dis_amd/tracking.py has the numpy counterpart of the same name."""
    _fields_ = [("min_len", C.c_int), ("min_std", C.c_float), ("max_std", C.c_float), ("max_step", C.c_float),
                ("max_step_share", C.c_float), ("min_camera", C.c_float), ("tests", C.c_uint)]

    def __init__(self, **kw):
        super().__init__()
        lib().ofdis_track_select_defaults(C.byref(self))
        for k, v in kw.items():
            assert k in dict(self._fields_), k
            setattr(self, k, v)

    @classmethod
    def of(cls, params):
        """None (the defaults), a TrackSelectParams of this module or of tracking.py"""
        if params is None or isinstance(params, cls):
            return params or cls()
        return cls(**{k: getattr(params, k) for k, _ in cls._fields_})


class OfdisError(RuntimeError):
    pass


def _prototypes():
    """include/ofdis.h as ctypes prototypes (abi.py).  The header is the tree's own: the library is only ever built in-tree."""
    try:
        return prototypes()
    except OSError as e:
        raise OfdisError(f"include/ofdis.h cannot be read ({e}): the binding takes every prototype from it") from e


ABI_SYMBOLS = list(_prototypes())  # every function include/ofdis.h declares
_lib = None


def lib():
    """Load libofdis_hip.so (built by of_dis_amd.build) and give every function the header's prototype.  Fails loudly when
    the library is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OfdisError(f"{LIB_PATH} is missing: run `python -m of_dis_amd.build` (no CPU fallback exists)")
        L = C.CDLL(LIB_PATH)
        if L.ofdis_version() != OFDIS_VERSION:  # a stale build: ofdis_get_tuning would write past / read garbage from our struct
            raise OfdisError(f"{LIB_PATH} has ABI version {L.ofdis_version()}, this binding expects {OFDIS_VERSION}: "
                             "rebuild with `python -m of_dis_amd.build`")
        _lib = bind(L, _prototypes())
    return _lib


def check(rc):
    if rc != 0:
        raise OfdisError(f"ofdis status {rc}: {lib().ofdis_last_error().decode()}")


def build_id():
    """ofdis_build_id(): the hash of the kernel sources + flags the loaded library was built from."""
    return lib().ofdis_build_id().decode()


def device_pci_bus_id(device):
    buf = C.create_string_buffer(32)
    check(lib().ofdis_device_pci_bus_id(device, buf, 32))
    return buf.value.decode()


def get_tuning():
    t = OfdisTuning()
    check(lib().ofdis_get_tuning(C.byref(t)))
    return t


def set_tuning(**kw):
    """Change kernel-selection knobs (ofdis_set_tuning); returns the previous settings (pass them to restore_tuning)."""
    old = get_tuning()
    new = get_tuning()
    for k, v in kw.items():
        setattr(new, k, v)
    check(lib().ofdis_set_tuning(C.byref(new)))
    lib().ofdis_flow_cache_clear()  # cached drop-in contexts were sized under the old settings
    return old


def restore_tuning(old):
    check(lib().ofdis_set_tuning(C.byref(old)))
    lib().ofdis_flow_cache_clear()


class Dev:
    """A device buffer owned through ofdis_dev_alloc / ofdis_dev_free."""

    def __init__(self, arr=None, nbytes=None):
        L = lib()
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            nbytes = arr.nbytes
        self.nbytes = int(nbytes)
        self.ptr = L.ofdis_dev_alloc(self.nbytes)
        if not self.ptr:
            raise OfdisError("device allocation failed")
        if arr is not None:
            check(L.ofdis_memcpy_h2d(self.ptr, arr.ctypes.data, self.nbytes))

    def get(self, shape, dtype=_f32):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        check(lib().ofdis_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().ofdis_dev_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Stream:
    """A non-blocking HIP stream owned through ofdis_stream_create / ofdis_stream_destroy (`.ptr` goes wherever the ABI takes
    a `stream`)."""

    def __init__(self):
        self.ptr = lib().ofdis_stream_create()
        if not self.ptr:
            raise OfdisError(f"ofdis_stream_create: {lib().ofdis_last_error().decode()}")

    def sync(self):
        check(lib().ofdis_sync(self.ptr))

    def close(self):
        if self.ptr:
            lib().ofdis_stream_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Event:
    """A HIP event owned through ofdis_event_create / ofdis_event_destroy: orders work across streams without the host."""

    def __init__(self):
        self.ptr = lib().ofdis_event_create()
        if not self.ptr:
            raise OfdisError(f"ofdis_event_create: {lib().ofdis_last_error().decode()}")

    def record(self, stream):
        check(lib().ofdis_event_record(self.ptr, stream.ptr if isinstance(stream, Stream) else stream))

    def wait(self, stream):
        """make `stream` wait for the last recorded point"""
        check(lib().ofdis_stream_wait_event(stream.ptr if isinstance(stream, Stream) else stream, self.ptr))

    def sync(self):
        check(lib().ofdis_event_sync(self.ptr))

    def close(self):
        if self.ptr:
            lib().ofdis_event_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostBuf:
    """Page-locked host memory (ofdis_host_alloc) seen as a numpy array: the source / destination of the asynchronous copies."""

    def __init__(self, shape, dtype=_f32):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = lib().ofdis_host_alloc(self.nbytes)
        if not self.ptr:
            raise OfdisError(f"ofdis_host_alloc: {lib().ofdis_last_error().decode()}")
        self.array = np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_uint8)), shape=(self.nbytes,)).view(dtype).reshape(shape)

    def free(self):
        if self.ptr:
            self.array = None
            lib().ofdis_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceCall:
    """One call of the library on host arrays: the device buffers of the call and what happens to them after it.

        with DeviceCall(stream) as c:
            check(lib().ofdis_x(c.input(a), c.input(mask_or_None), n, c.output(shape, dtype, want), c.work(nbytes), nbytes, stream))
            return c.results()

    input, output and work each hand back the device pointer that goes into the C call, or None for NULL, so a wrapper names
    them in the call's own argument order.  results() synchronises `stream` once, downloads the outputs in the order they
    were declared (None where one was not wanted) and releases every buffer; nothing is released before that sync.  Leaving
    the block releases them as well, so an OfdisError of the call leaks nothing.

    own=False is the form of the Batch methods that are given device pointers: output() then takes the caller's pointer (or a
    false value for NULL) as `want` and passes it through, and results() downloads nothing and returns None; it synchronises
    only if an input was uploaded, which must outlive the launch."""
    MIN_BYTES = 8  # the least allocation of an output or a work buffer: none of zero bytes (kernels write what the shapes say)

    def __init__(self, stream=None, own=True):
        self.stream, self.own = stream, own
        self._devs = []  # every buffer of the call
        self._outs = []  # (buffer or None, shape, dtype) of every output, in declaration order
        self._uploaded = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()

    def _dev(self, arr=None, nbytes=None):
        self._uploaded |= arr is not None
        self._devs.append(Dev(arr, nbytes))
        return self._devs[-1]

    def input(self, arr):
        """the device copy of a host array, coerced by the caller: its pointer; None for None"""
        return None if arr is None else self._dev(arr).ptr

    def output(self, shape, dtype=_f32, want=True, fill=None, over=None):
        """An output of `shape` and `dtype`: its pointer, or None where it is not wanted.  fill: the contents it starts from, a host
        array of that many elements (an array the call updates in place is an output filled with it).  over: the pointer
        input() gave for the input whose device array the call is to overwrite with this output."""
        if not self.own:
            return want if want and want is not True else None  # (a bare True is no pointer)
        dev = None
        if want and over is not None:
            dev = next(d for d in self._devs if d.ptr == over)
        elif want and fill is not None:
            dev = self._dev(np.ascontiguousarray(fill, dtype).reshape(shape))
        elif want:
            dev = self._dev(nbytes=max(self.MIN_BYTES, int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize))
        self._outs.append((dev, shape, dtype))
        return dev.ptr if dev else None

    def work(self, nbytes):
        """a work buffer of at least `nbytes` bytes: its pointer"""
        return self._dev(nbytes=max(self.MIN_BYTES, int(nbytes))).ptr

    def results(self):
        """After the call: the tuple of the outputs as host arrays, in declaration order; None with own=False."""
        try:
            if self.own or self._uploaded:
                check(lib().ofdis_sync(self.stream))
            if not self.own:
                return None
            return tuple(dev.get(shape, dtype) if dev else None for dev, shape, dtype in self._outs)
        finally:
            self.release()

    def release(self):
        for dev in self._devs:
            dev.free()
        self._devs = []


def _f(a):
    return np.ascontiguousarray(a, dtype=_f32)


def _pair_flows(flow_fw, flow_rev=None):
    """flow_fw [npairs, h, w, 2] float32 and its reverse partner, the same shape or None -> (flow_fw, flow_rev, npairs, h, w)"""
    flow_fw = _f(flow_fw)
    assert flow_fw.ndim == 4 and flow_fw.shape[-1] == 2, flow_fw.shape
    if flow_rev is not None:
        flow_rev = _f(flow_rev)
        assert flow_rev.shape == flow_fw.shape, (flow_rev.shape, flow_fw.shape)
    return (flow_fw, flow_rev) + flow_fw.shape[:3]


def _mask(mask, shape):
    """an optional uint8 mask of `shape`: the array to upload, or None for None"""
    if mask is None:
        return None
    mask = np.ascontiguousarray(mask, np.uint8)
    assert mask.shape == shape, (mask.shape, shape)
    return mask


# ------------------------------------------------------------------ per-function entry points (numpy in/out)
def image_warp(src, wx, wy):
    """src [B,noc,h,w], wx/wy [B,h,w] -> dst [B,noc,h,w], mask [B,h,w]"""
    src, wx, wy = _f(src), _f(wx), _f(wy)
    B, noc, h, w = src.shape
    with DeviceCall() as c:
        check(lib().ofdis_image_warp(c.output(src.shape), c.output(wx.shape), c.input(src), c.input(wx), c.input(wy), w, h, noc, B,
                                     None))
        return c.results()


def get_derivatives(im1, im2w):
    """im1, im2w [B,noc,h,w] -> [B,8,noc,h,w]"""
    im1, im2w = _f(im1), _f(im2w)
    B, noc, h, w = im1.shape
    with DeviceCall() as c:
        check(lib().ofdis_get_derivatives(c.output((B, 8, noc, h, w)), c.input(im1), c.input(im2w), w, h, noc, B, None))
        return c.results()[0]


def tv_system(mask, wx, wy, du, dv, derivs, tv_alpha, tv_gamma, tv_delta):
    """-> [B,7,h,w] = a11,a12,a22,b1,b2,smooth_horiz,smooth_vert"""
    mask, wx, wy, du, dv, derivs = [_f(x) for x in (mask, wx, wy, du, dv, derivs)]
    B, h, w = mask.shape
    noc = derivs.shape[2]
    with DeviceCall() as c:
        check(lib().ofdis_tv_system(c.output((B, 7, h, w)), *[c.input(x) for x in (mask, wx, wy, du, dv, derivs)], tv_alpha,
                                    tv_gamma, tv_delta, w, h, noc, B, None))
        return c.results()[0]


def sor_coupled(du, dv, sys, iterations, omega):
    """du, dv [B,h,w]; sys [B,7,h,w] -> new du, dv"""
    du, dv, sys = _f(du), _f(dv), _f(sys)
    B, h, w = du.shape
    with DeviceCall() as c:
        check(lib().ofdis_sor_coupled(c.output(du.shape, fill=du), c.output(dv.shape, fill=dv), c.input(sys), iterations, omega,
                                      w, h, B, None))
        return c.results()


def patchgrid_level(p, level, im_a, im_a_dx, im_a_dy, im_b, flow_prev=None):
    """Planes [B,tmp_h,tmp_w,noc]; flow_prev [B,h/2,w/2,2] or None -> p [B,nop,2], flow [B,h,w,2]"""
    im_a, im_a_dx, im_a_dy, im_b = [_f(x) for x in (im_a, im_a_dx, im_a_dy, im_b)]
    flow_prev = _f(flow_prev) if flow_prev is not None else None
    B = im_a.shape[0]
    w, h = p.level_size(level)
    nw, nh = p.grid(level)
    nop = nw * nh
    with DeviceCall() as c:
        check(lib().ofdis_patchgrid_level(C.byref(p), level, *[c.input(x) for x in (im_a, im_a_dx, im_a_dy, im_b, flow_prev)],
                                          c.output((B, nop, 2)), c.output((B, h, w, p.nop)), B, None))
        return c.results()


def varref_level(p, level, im_a, im_b, flow):
    """im_a, im_b [B,tmp_h,tmp_w,noc]; flow [B,h,w,2] -> refined flow"""
    im_a, im_b, flow = _f(im_a), _f(im_b), _f(flow)
    B = im_a.shape[0]
    with DeviceCall() as c:
        check(lib().ofdis_varref_level(C.byref(p), level, c.input(im_a), c.input(im_b), c.output(flow.shape, fill=flow), B, None))
        return c.results()[0]


def _ptr_array(planes, n):
    arr = (FP * n)()
    for i in range(n):
        arr[i] = planes[i].ctypes.data_as(FP) if (i < len(planes) and planes[i] is not None) else None
    return arr


def flow(p, pyr_a, pyr_a_dx, pyr_a_dy, pyr_b, initflow=None, pyr_b_dx=None, pyr_b_dy=None):
    """ofdis_flow(): the drop-in for OFC::OFClass::OFClass with host pyramids (lists over levels 0..sc_f)."""
    n = p.sc_f + 1
    keep = [[_f(x) if x is not None else None for x in pl] for pl in (pyr_a, pyr_a_dx, pyr_a_dy, pyr_b)]
    keep_b = [[_f(x) if x is not None else None for x in pl] for pl in (pyr_b_dx, pyr_b_dy) if pl is not None]
    w, h = p.level_size(p.sc_l)
    out = np.zeros((h, w, p.nop), _f32)
    nullarr = C.cast(None, C.POINTER(FP))
    bdx = _ptr_array(keep_b[0], n) if len(keep_b) == 2 else nullarr
    bdy = _ptr_array(keep_b[1], n) if len(keep_b) == 2 else nullarr
    check(lib().ofdis_flow(C.byref(p), _ptr_array(keep[0], n), _ptr_array(keep[1], n), _ptr_array(keep[2], n),
                           _ptr_array(keep[3], n), bdx, bdy, out.ctypes.data_as(FP),
                           _f(initflow).ctypes.data_as(FP) if initflow is not None else None))
    return out


def fb_check(flow, other, alpha=FB_ALPHA, beta=FB_BETA):
    """ofdis_fb_check on the device: flow, other [..., h, w, 2] float32 (the same shape; leading axes are frames) ->
    uint8 mask [..., h, w] of FB_CONSISTENT / FB_INCONSISTENT / FB_OUTSIDE for every pixel of `flow`."""
    flow, other = _f(flow), _f(other)
    assert flow.shape == other.shape and flow.ndim >= 3 and flow.shape[-1] == 2, (flow.shape, other.shape)
    h, w = flow.shape[-3:-1]
    n = int(np.prod(flow.shape[:-3], dtype=np.int64))
    with DeviceCall() as c:
        check(lib().ofdis_fb_check(c.input(flow), c.input(other), c.output(flow.shape[:-1], np.uint8), n, w, h, alpha, beta, None))
        return c.results()[0]


def lr_check(disp, other, alpha=FB_ALPHA, beta=FB_BETA):
    """ofdis_lr_check on the device: disp, other [..., h, w] float32 (the same shape; leading axes are frames), the
    displacement in x towards the other view -> uint8 mask [..., h, w] of FB_* codes for every pixel of `disp`."""
    disp, other = _f(disp), _f(other)
    assert disp.shape == other.shape and disp.ndim >= 2, (disp.shape, other.shape)
    h, w = disp.shape[-2:]
    n = int(np.prod(disp.shape[:-2], dtype=np.int64))
    with DeviceCall() as c:
        check(lib().ofdis_lr_check(c.input(disp), c.input(other), c.output(disp.shape, np.uint8), n, w, h, alpha, beta, None))
        return c.results()[0]


def disparity_fill(disp, mask, mode, in_place=False):
    """ofdis_disparity_fill on the device: disp [..., h, w] float32, mask the same shape uint8 -> filled disparities.
    in_place: `out` is `disp` itself (the library allows it)."""
    disp = _f(disp)
    mask = np.ascontiguousarray(mask, np.uint8)
    assert disp.shape == mask.shape and disp.ndim >= 2, (disp.shape, mask.shape)
    h, w = disp.shape[-2:]
    n = int(np.prod(disp.shape[:-2], dtype=np.int64))
    with DeviceCall() as c:
        pd = c.input(disp)
        check(lib().ofdis_disparity_fill(pd, c.input(mask), c.output(disp.shape, over=pd if in_place else None), n, w, h, mode,
                                         None))
        return c.results()[0]


def _enc_dtype(enc):
    """the dtype of an output in the encoding `enc`; bytes for an unknown type (ofdis_encoding_bytes gives 0), which the library
    rejects"""
    return enc.dtype if lib().ofdis_encoding_bytes(enc.type) else np.dtype(np.uint8)


def encode(array, enc):
    """ofdis_encode on the device: a float32 array of any shape -> the same shape in enc.dtype."""
    a = _f(array)
    with DeviceCall() as c:
        check(lib().ofdis_encode(c.input(a), c.output(a.shape, _enc_dtype(enc)), a.size, C.byref(enc), None))
        return c.results()[0]


def _times(times):
    t = np.ascontiguousarray(np.atleast_1d(np.asarray(times, _f32)).ravel())
    return t, t.ctypes.data_as(FP)


def interpolate(img_a, img_b, flow_fw, flow_rev, times, mask_fw=None, mask_rev=None):
    """ofdis_interpolate on the device: frames img_a, img_b uint8 [..., h, w] (gray) or [..., h, w, 3]; flows [..., h, w, 2]
    float32 (A -> B and B -> A); masks uint8 [..., h, w] or None (all consistent); times: a sequence of 1..INTERP_MAX_TIMES
    values in [0, 1].  Returns uint8 [..., len(times), h, w] (+ [3]); the leading axes are frames."""
    flow_fw, flow_rev = _f(flow_fw), _f(flow_rev)
    assert flow_fw.shape == flow_rev.shape and flow_fw.ndim >= 3 and flow_fw.shape[-1] == 2, (flow_fw.shape, flow_rev.shape)
    lead, (h, w) = flow_fw.shape[:-3], flow_fw.shape[-3:-1]
    img_a, img_b = np.ascontiguousarray(img_a, np.uint8), np.ascontiguousarray(img_b, np.uint8)
    assert img_a.shape == img_b.shape, (img_a.shape, img_b.shape)
    noc = 1 if img_a.shape == flow_fw.shape[:-1] else 3
    assert img_a.shape == flow_fw.shape[:-1] + ((3,) if noc == 3 else ()), (img_a.shape, flow_fw.shape)
    n = int(np.prod(lead, dtype=np.int64))
    t, tp = _times(times)
    masks = [_mask(m, flow_fw.shape[:-1]) for m in (mask_fw, mask_rev)]
    shape = lead + (t.size, h, w) + ((3,) if noc == 3 else ())
    with DeviceCall() as c:
        check(lib().ofdis_interpolate(*[c.input(x) for x in (img_a, img_b, flow_fw, flow_rev, *masks)], c.output(shape, np.uint8),
                                      n, w, h, noc, tp, t.size, None))
        return c.results()[0]


def _track_inputs(seeds, seed_frame):
    seeds = _f(seeds)
    assert seeds.ndim == 2 and seeds.shape[1] == 2, seeds.shape
    if seed_frame is not None:
        seed_frame = np.ascontiguousarray(seed_frame, np.int32)
        assert seed_frame.shape == (seeds.shape[0],), (seed_frame.shape, seeds.shape)
    return seeds, seed_frame


def track_points(flow_fw, flow_rev, seeds, seed_frame=None, max_steps=0, alpha=FB_ALPHA, beta=FB_BETA):
    """ofdis_track_points on the device: flow_fw [npairs, h, w, 2] float32 (frame k -> k + 1), flow_rev the same shape
    (frame k + 1 -> k) or None (no consistency test), seeds [npoints, 2] float32 (x, y), seed_frame [npoints] int32 or None
    (all 0) -> (tracks [npairs + 1, npoints, 2] float32, counts [npoints] int32).  of_dis_amd/tracking.py: track_ref is the
    numpy statement of the same arithmetic."""
    flow_fw, flow_rev, npairs, h, w = _pair_flows(flow_fw, flow_rev)
    seeds, seed_frame = _track_inputs(seeds, seed_frame)
    n = seeds.shape[0]
    with DeviceCall() as c:
        check(lib().ofdis_track_points(c.input(flow_fw), c.input(flow_rev), npairs, w, h, c.input(seeds), c.input(seed_frame), n,
                                       max_steps, alpha, beta, c.output((npairs + 1, n, 2)), c.output((n,), np.int32), None))
        return c.results()


def dense_tracks_cells(width, height, stride):
    """ofdis_dense_tracks_cells: (ncx, ncy) of the seed grid, (0, 0) for rejected sizes"""
    ncx, ncy = C.c_int(-1), C.c_int(-1)
    n = lib().ofdis_dense_tracks_cells(width, height, stride, C.byref(ncx), C.byref(ncy))
    assert n == ncx.value * ncy.value, (n, ncx.value, ncy.value)
    return ncx.value, ncy.value


def _clip_frames(frames, n, h, w):
    frames = np.ascontiguousarray(frames, np.uint8)
    noc = 1 if frames.ndim == 3 else 3
    assert frames.shape == (n, h, w) + ((3,) if noc == 3 else ()), (frames.shape, (n, h, w))
    return frames, noc


def seed_texture(frames, stride, window, min_eig):
    """ofdis_seed_texture on the device: frames uint8 [n, h, w] (gray) or [n, h, w, 3] -> uint8 [n, ncy, ncx], 1 where the cell
    centre passes the texture test.  of_dis_amd/tracking.py: seed_texture_ref is the numpy statement of the same arithmetic."""
    frames = np.ascontiguousarray(frames, np.uint8)
    n, h, w = frames.shape[:3]
    frames, noc = _clip_frames(frames, n, h, w)
    ncx, ncy = dense_tracks_cells(w, h, stride)
    with DeviceCall() as c:
        check(lib().ofdis_seed_texture(c.input(frames), n, w, h, noc, stride, window, min_eig, c.output((n, ncy, ncx), np.uint8),
                                       None))
        return c.results()[0]


def _dense_lmax(max_len, npairs):
    return min(max_len, npairs) if max_len else npairs


def _dense_specs(lmax, slots):
    """(shape, dtype) of the four outputs of a dense_tracks call with `slots` track slots: tracks, start, len, info"""
    return [((lmax + 1, slots, 2), _f32), ((slots,), np.int32), ((slots,), np.int32), ((2,), np.int64)]


def _dense_declare(c, lmax, slots):
    """those four outputs declared on the DeviceCall `c`: their pointers"""
    return tuple(c.output(shape, dtype) for shape, dtype in _dense_specs(lmax, slots))


def _dense_cut(arrays, lmax, max_tracks):
    """the four host arrays of such a call -> (tracks [lmax + 1, ntracks, 2], start [ntracks], len [ntracks], info [2]): the
    slots the call wrote"""
    tracks, start, length, info = arrays
    n = int(info[0])
    assert 0 <= n <= max_tracks and tracks.shape[0] == lmax + 1, (info, tracks.shape)
    return np.ascontiguousarray(tracks[:, :n]), start[:n].copy(), length[:n].copy(), info


def _dense_outputs(lmax, max_tracks):
    """The same four outputs as device arrays of the caller's, outside a DeviceCall: tests/test_gpu_level_routes.py hands their
    pointers to a launch hook, synchronises and reads them back with _dense_results."""
    return tuple(Dev(nbytes=int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize)
                 for shape, dtype in _dense_specs(lmax, max_tracks))


def _dense_results(devs, lmax, max_tracks):
    """the device arrays of _dense_outputs, after the caller's sync -> what _dense_cut returns"""
    return _dense_cut([d.get(shape, dtype) for d, (shape, dtype) in zip(devs, _dense_specs(lmax, max_tracks))], lmax, max_tracks)


def _track_info(n):
    """the `info` ofdis_dense_tracks writes, for n tracks on the host: (ntracks, dropped)"""
    return np.array([n, 0], np.int64)


def dense_tracks(frames, flow_fw, flow_rev, stride, window, min_eig, max_len=15, max_tracks=None, alpha=FB_ALPHA, beta=FB_BETA):
    """ofdis_dense_tracks on the device: frames uint8 [npairs + 1, h, w] (gray) or [npairs + 1, h, w, 3], flow_fw / flow_rev
    [npairs, h, w, 2] float32 (flow_rev None: no consistency test) -> (tracks [Lmax + 1, ntracks, 2] float32, start [ntracks]
    int32, len [ntracks] int32, info int64 [2] = (ntracks, dropped)): the slots below ntracks.  max_tracks None: room for every
    seed (npairs x cells, at most DT_MAX_TRACKS).  of_dis_amd/tracking.py: dense_tracks_ref is the numpy statement of the same
    process."""
    flow_fw, flow_rev, npairs, h, w = _pair_flows(flow_fw, flow_rev)
    frames, noc = _clip_frames(frames, npairs + 1, h, w)
    ncx, ncy = dense_tracks_cells(w, h, stride)
    if max_tracks is None:
        max_tracks = max(1, min(npairs * ncx * ncy, DT_MAX_TRACKS))
    lmax = _dense_lmax(max_len, npairs)
    wb = lib().ofdis_dense_tracks_work_bytes(npairs, w, h, stride)
    with DeviceCall() as c:
        check(lib().ofdis_dense_tracks(c.input(frames), c.input(flow_fw), c.input(flow_rev), npairs, w, h, noc, stride, window,
                                       min_eig, max_len, alpha, beta, max_tracks,
                                       *_dense_declare(c, lmax, max(1, min(max_tracks, DT_MAX_TRACKS))), c.work(wb), wb, None))
        return _dense_cut(c.results(), lmax, max_tracks)


def track_select_work_bytes(max_tracks):
    """ofdis_track_select_work_bytes: the work buffer of track_select_dev; 0 for rejected sizes."""
    return lib().ofdis_track_select_work_bytes(max_tracks)


def track_select_dev(tracks_ptr, start_ptr, len_ptr, info_ptr, lmax, max_tracks, max_tracks_out, tracks_out_ptr, start_out_ptr,
                     len_out_ptr, info_out_ptr, work_ptr, work_bytes, models_ptr=None, npairs=0, width=0, height=0, params=None,
                     code_ptr=None, counts_ptr=None, index_ptr=None, shape_out_ptr=None, stream=None, nparam=6):
    """ofdis_track_select on device pointers: the arrays ofdis_dense_tracks wrote stay where they are; the selected set
    (tracks_out [lmax + 1][max_tracks_out][2], start_out, len_out [max_tracks_out], info_out [2]) has the same layout and feeds
    track_descriptors_dev, track_bof_dev and codebook_train_dev unchanged.  models [npairs][6] float64 of a width x height
    clip, code [max_tracks] uint8, counts [7] int64, index [max_tracks_out] int32 and shape_out [max_tracks_out][lmax][2] are
    optional.  nparam=8: models [npairs][8] of projective_motion (ofdis_track_select_projective).  Enqueues on `stream` and
    returns; nothing synchronises with the host."""
    p = TrackSelectParams.of(params)
    assert nparam in (6, 8), nparam
    call = lib().ofdis_track_select if nparam == 6 else lib().ofdis_track_select_projective
    check(call(tracks_ptr, start_ptr, len_ptr, info_ptr, lmax, max_tracks, models_ptr, npairs, width, height,
               C.byref(p), code_ptr, counts_ptr, max_tracks_out, tracks_out_ptr, start_out_ptr, len_out_ptr,
               info_out_ptr, index_ptr, shape_out_ptr, work_ptr, work_bytes, stream))


def track_select(tracks, start, length, models=None, size=None, params=None, max_out=None, shape=True):
    """ofdis_track_select on host arrays: tracks [Lmax + 1, ntracks, 2], start, length [ntracks] as dense_tracks returns them;
    models float64 [npairs, 6] as global_motion returns them -- or [npairs, 8] as projective_motion does, which routes to
    ofdis_track_select_projective -- with size = (width, height) of their frames, or None; params a
    TrackSelectParams (None: the defaults); max_out the slots of the output set (None: room for every track) -> (code uint8
    [ntracks], counts int64 [7], tracks_out [Lmax + 1, nkept, 2], start_out, len_out int32 [nkept], info_out int64 [2] =
    (nkept written, dropped), index int32 [nkept], shape_out float32 [nkept, Lmax, 2] or None with shape=False): the outputs
    cut to the slots the call wrote.  of_dis_amd/tracking.py: track_select_ref is the numpy statement of the same definition."""
    tracks = _f(tracks)
    assert tracks.ndim == 3 and tracks.shape[0] >= 2 and tracks.shape[2] == 2, tracks.shape
    lmax, n = tracks.shape[0] - 1, tracks.shape[1]
    start, length = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(length, np.int32)
    assert start.shape == length.shape == (n,), (start.shape, length.shape, n)
    slots = max(n, 1)  # (the library takes no empty array)
    out = slots if max_out is None else int(max_out)
    oslots = max(out, 1)
    npairs, w, h, nparam = 0, 0, 0, 6
    if models is not None:
        models = np.ascontiguousarray(models, np.float64)
        nparam = 8 if models.ndim == 2 and models.shape[1] == 8 else 6
        models = models.reshape(-1, nparam)
        npairs, (w, h) = len(models), size
    if not n:
        tracks, start, length = np.zeros((lmax + 1, 1, 2), _f32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    wb = track_select_work_bytes(slots)
    with DeviceCall() as c:  # (in the order of track_select_dev's parameters)
        track_select_dev(*[c.input(a) for a in (tracks, start, length, _track_info(n))], lmax, slots, out,
                         *_dense_declare(c, lmax, oslots), c.work(wb), wb, c.input(models), npairs, w, h, params,
                         c.output((slots,), np.uint8), c.output((7,), np.int64), c.output((oslots,), np.int32),
                         c.output((oslots, lmax, 2), _f32, shape), nparam=nparam)
        *dense, code, counts, index, shape_out = c.results()
    tracks_out, start_out, len_out, info = _dense_cut(dense, lmax, out)
    k = int(info[0])
    return (code[:n].copy(), counts, tracks_out, start_out, len_out, info, index[:k].copy(),
            shape_out[:k].copy() if shape else None)


def track_descriptor_dims(patch, nxy, nt):
    """ofdis_track_descriptor_dims: D = 33 * nxy^2 * nt, 0 for rejected parameters"""
    return lib().ofdis_track_descriptor_dims(patch, nxy, nt)


def track_descriptors_dev(frames_ptr, flow_ptr, npairs, width, height, noc, tracks_ptr, start_ptr, len_ptr, info_ptr, lmax,
                          max_tracks, patch, nxy, nt, min_flow, hist_ptr, shape_ptr=None, stream=None):
    """ofdis_track_descriptors on device pointers: the arrays ofdis_dense_tracks wrote (tracks [lmax + 1][max_tracks][2], start,
    len [max_tracks], info) stay where they are; hist [max_tracks][D] uint32 and shape [max_tracks][lmax][2] float32 (or None)
    are the caller's.  Enqueues on `stream` and returns; nothing synchronises with the host."""
    check(lib().ofdis_track_descriptors(frames_ptr, flow_ptr, npairs, width, height, noc, tracks_ptr, start_ptr, len_ptr, info_ptr,
                                        lmax, max_tracks, patch, nxy, nt, min_flow, hist_ptr, shape_ptr, stream))


def track_descriptors(frames, flow_fw, tracks, start, length, patch, nxy, nt, min_flow, shape=True):
    """ofdis_track_descriptors on host arrays: frames uint8 [npairs + 1, h, w] (gray) or [npairs + 1, h, w, 3], flow_fw
    [npairs, h, w, 2] float32 (or the residual flow of motion_compensate), tracks [Lmax + 1, ntracks, 2], start, length
    [ntracks] as dense_tracks returns them -> (hist uint32 [ntracks, D], shape float32 [ntracks, Lmax, 2] or None with
    shape=False).  of_dis_amd/tracking.py: track_descriptors_ref is the numpy statement of the same definition."""
    flow_fw, _, npairs, h, w = _pair_flows(flow_fw)
    frames, noc = _clip_frames(frames, npairs + 1, h, w)
    tracks = _f(tracks)
    assert tracks.ndim == 3 and tracks.shape[0] >= 2 and tracks.shape[2] == 2, tracks.shape
    lmax, n = tracks.shape[0] - 1, tracks.shape[1]
    start, length = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(length, np.int32)
    assert start.shape == length.shape == (n,), (start.shape, length.shape, n)
    D = track_descriptor_dims(patch, nxy, nt)
    slots = max(n, 1)  # (the library takes no empty array)
    if not n:
        tracks, start, length = np.zeros((lmax + 1, 1, 2), _f32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    with DeviceCall() as c:
        track_descriptors_dev(c.input(frames), c.input(flow_fw), npairs, w, h, noc,
                              *[c.input(a) for a in (tracks, start, length, _track_info(n))], lmax, slots, patch, nxy, nt, min_flow,
                              c.output((slots, D), np.uint32), c.output((slots, lmax, 2), _f32, shape))
        hist, shape_out = c.results()
    return hist[:n].copy(), shape_out[:n].copy() if shape else None


def _bof_inputs(rows, D, dtype):
    """[ntracks, D] rows of `dtype` -> (the rows to upload: one idle slot for an empty array, ntracks, slots)"""
    rows = np.ascontiguousarray(rows, dtype)
    assert rows.ndim == 2 and rows.shape[1] == D, (rows.shape, D)
    n = rows.shape[0]
    return rows if n else np.zeros((1, D), dtype), n, max(n, 1)


def _bof_len(length, n, optional=False):
    """length [ntracks] int32 -> the array to upload: one idle slot for an empty array.  optional: None stays None (the k-means
    calls: every track is a member)"""
    if optional and length is None:
        return None
    length = np.ascontiguousarray(length, np.int32)
    assert length.shape == (n,), (length.shape, n)
    return length if n else np.zeros(1, np.int32)


def _bof_codebook(codebook, D):
    codebook = np.ascontiguousarray(codebook, np.uint8)
    assert codebook.ndim == 2 and codebook.shape[1] == D and 1 <= codebook.shape[0] <= BOF_MAX_WORDS, (codebook.shape, D)
    return codebook


def descriptor_normalize(hist, nxy, nt):
    """ofdis_descriptor_normalize on host arrays: hist uint32 [ntracks, 33 * nxy^2 * nt] -> desc uint8 of the same shape, every
    channel an 8-bit RootSIFT descriptor in units of 1 / BOF_SCALE.  of_dis_amd/tracking.py: normalize_descriptors_u8."""
    D = 33 * nxy * nxy * nt
    hist, n, slots = _bof_inputs(hist, D, np.uint32)
    with DeviceCall() as c:
        check(lib().ofdis_descriptor_normalize(c.input(hist), c.input(_track_info(n)), slots, nxy, nt,
                                               c.output((slots, D), np.uint8), None))
        return c.results()[0][:n].copy()


def codebook_assign(desc, codebook, nxy, nt):
    """ofdis_codebook_assign on host arrays: desc uint8 [ntracks, D], codebook uint8 [nwords, D] -> (words, dist), each int32
    [ntracks, 4]: per channel (HOG, HOF, MBHx, MBHy) the nearest word, the lowest index on a tie, and its squared distance.
    of_dis_amd/tracking.py: codebook_assign_ref."""
    D = 33 * nxy * nxy * nt
    desc, n, slots = _bof_inputs(desc, D, np.uint8)
    codebook = _bof_codebook(codebook, D)
    with DeviceCall() as c:
        check(lib().ofdis_codebook_assign(c.input(desc), c.input(_track_info(n)), slots, nxy, nt, c.input(codebook), len(codebook),
                                          c.output((slots, 4), np.int32), c.output((slots, 4), np.int32), None))
        words, dist = c.results()
    return words[:n].copy(), dist[:n].copy()


def bof_histogram(words, length, nwords, min_len=1):
    """ofdis_bof_histogram on host arrays: words int32 [ntracks, 4], length int32 [ntracks] -> bof uint32 [4, nwords], the tracks
    of at least min_len points counted by their words.  of_dis_amd/tracking.py: bof_ref."""
    words, n, slots = _bof_inputs(words, 4, np.int32)
    with DeviceCall() as c:
        check(lib().ofdis_bof_histogram(c.input(words), c.input(_bof_len(length, n)), c.input(_track_info(n)), slots, nwords,
                                        min_len, c.output((4, nwords), np.uint32), None))
        return c.results()[0]


def track_bof_dev(hist_ptr, len_ptr, info_ptr, max_tracks, nxy, nt, codebook_ptr, nwords, min_len, bof_ptr, words_ptr=None,
                  stream=None):
    """ofdis_track_bof on device pointers: hist [max_tracks][D] uint32 as ofdis_track_descriptors wrote it, len and info as
    ofdis_dense_tracks did, codebook [nwords][D] uint8 -> bof [4][nwords] uint32 and, where asked for, words [max_tracks][4]
    int32.  Enqueues on `stream` and returns; nothing synchronises with the host."""
    check(lib().ofdis_track_bof(hist_ptr, len_ptr, info_ptr, max_tracks, nxy, nt, codebook_ptr, nwords, min_len, bof_ptr, words_ptr,
                                stream))


def track_bof(hist, length, codebook, nxy, nt, min_len=1, words=False):
    """ofdis_track_bof on host arrays: hist uint32 [ntracks, D] and length [ntracks] (track_descriptors, dense_tracks), codebook
    uint8 [nwords, D] -> bof uint32 [4, nwords], or (bof, words int32 [ntracks, 4]) with words=True: normalisation, assignment
    and counting in one pass, bit-identical to descriptor_normalize -> codebook_assign -> bof_histogram."""
    D = 33 * nxy * nxy * nt
    hist, n, slots = _bof_inputs(hist, D, np.uint32)
    codebook = _bof_codebook(codebook, D)
    with DeviceCall() as c:
        track_bof_dev(c.input(hist), c.input(_bof_len(length, n)), c.input(_track_info(n)), slots, nxy, nt, c.input(codebook),
                      len(codebook), min_len, c.output((4, len(codebook)), np.uint32), c.output((slots, 4), np.int32, words))
        bof, words_out = c.results()
    return (bof, words_out[:n].copy()) if words else bof


def codebook_train_work_bytes(max_tracks, nxy, nt, nwords):
    """ofdis_codebook_train_work_bytes: the work buffer of codebook_update / codebook_train_dev; 0 for rejected sizes."""
    return int(lib().ofdis_codebook_train_work_bytes(max_tracks, nxy, nt, nwords))


def codebook_seed(desc, nxy, nt, nwords, length=None, min_len=1):
    """ofdis_codebook_seed on host arrays: desc uint8 [ntracks, D], length int32 [ntracks] or None -> codebook uint8 [nwords, D],
    row k the descriptor of the first track of at least min_len points at or after slot floor((2 k + 1) ntracks / (2 nwords)),
    cyclically; all zero without such a track.  of_dis_amd/tracking.py: codebook_seed_ref."""
    D = 33 * nxy * nxy * nt
    desc, n, slots = _bof_inputs(desc, D, np.uint8)
    with DeviceCall() as c:
        check(lib().ofdis_codebook_seed(c.input(desc), c.input(_bof_len(length, n, optional=True)), c.input(_track_info(n)), slots,
                                        nxy, nt, nwords, min_len, c.output((nwords, D), np.uint8), None))
        return c.results()[0]


def codebook_update(desc, words, codebook, nxy, nt, length=None, min_len=1):
    """ofdis_codebook_update on host arrays: desc uint8 [ntracks, D], words int32 [ntracks, 4], codebook uint8 [nwords, D] ->
    (codebook, counts uint32 [4, nwords]): per channel every word with members becomes their mean, rounded half up; a word
    without members keeps its bytes.  of_dis_amd/tracking.py: codebook_update_ref."""
    D = 33 * nxy * nxy * nt
    desc, n, slots = _bof_inputs(desc, D, np.uint8)
    codebook = _bof_codebook(codebook, D)
    words = np.ascontiguousarray(words, np.int32)
    assert words.shape == (n, 4), (words.shape, n)
    words = words if n else np.zeros((1, 4), np.int32)
    nwords = len(codebook)
    wb = codebook_train_work_bytes(slots, nxy, nt, nwords)
    with DeviceCall() as c:
        check(lib().ofdis_codebook_update(c.input(desc), c.input(words), c.input(_bof_len(length, n, optional=True)),
                                          c.input(_track_info(n)), slots, nxy, nt, nwords, min_len,
                                          c.output((nwords, D), np.uint8, fill=codebook), c.output((4, nwords), np.uint32),
                                          c.work(wb), wb, None))
        return c.results()


def codebook_train_dev(desc_ptr, len_ptr, info_ptr, max_tracks, nxy, nt, nwords, min_len, iters, codebook_ptr, words_ptr, counts_ptr,
                       stats_ptr, work_ptr, work_bytes, stream=None):
    """ofdis_codebook_train on device pointers: desc [max_tracks][D] uint8 as ofdis_descriptor_normalize wrote it, len (or None)
    and info as ofdis_dense_tracks did, codebook [nwords][D] uint8 in/out -> words [max_tracks][4] int32, counts [4][nwords]
    uint32 and, where asked for, stats [iters][4][2] int64.  Enqueues iters x (assignment + update) on `stream` and returns;
    nothing synchronises with the host."""
    check(lib().ofdis_codebook_train(desc_ptr, len_ptr, info_ptr, max_tracks, nxy, nt, nwords, min_len, iters, codebook_ptr,
                                     words_ptr, counts_ptr, stats_ptr, work_ptr, work_bytes, stream))


def codebook_train(desc, codebook, nxy, nt, iters, length=None, min_len=1):
    """ofdis_codebook_train on host arrays: desc uint8 [ntracks, D], codebook uint8 [nwords, D] (codebook_seed, or any seeding
    of the caller's) -> (codebook, words int32 [ntracks, 4], counts uint32 [4, nwords], stats int64 [iters, 4, 2]) after iters
    rounds of Lloyd's algorithm; stats[t][c] = (the members whose word changed, the sum of their squared distances).  words and
    counts belong to the last assignment, taken before the last update.  of_dis_amd/tracking.py: codebook_train_ref."""
    D = 33 * nxy * nxy * nt
    desc, n, slots = _bof_inputs(desc, D, np.uint8)
    codebook = _bof_codebook(codebook, D)
    nwords = len(codebook)
    wb = codebook_train_work_bytes(slots, nxy, nt, nwords)
    with DeviceCall() as c:
        codebook_train_dev(c.input(desc), c.input(_bof_len(length, n, optional=True)), c.input(_track_info(n)), slots, nxy, nt,
                           nwords, min_len, iters, c.output((nwords, D), np.uint8, fill=codebook), c.output((slots, 4), np.int32),
                           c.output((4, nwords), np.uint32), c.output((iters, 4, 2), np.int64), c.work(wb), wb)
        codebook, words, counts, stats = c.results()
    return codebook, words[:n].copy(), counts, stats


def temporal_filter(frames, flow_fw, flow_rev, mask_fw=None, mask_rev=None, wn=1.0, tau=np.inf, support=True):
    """ofdis_temporal_filter on the device: frames uint8 [npairs + 1, h, w] (gray) or [npairs + 1, h, w, 3]; flow_fw / flow_rev
    [npairs, h, w, 2] float32 (frame k -> k + 1 and frame k + 1 -> k); masks uint8 [npairs, h, w] or None (all consistent).
    Returns (out, the shape of frames; support uint8 [npairs + 1, h, w], or None with support=False: passed as NULL).
    of_dis_amd/temporal.py: temporal_filter_ref is the numpy statement of the same arithmetic."""
    flow_fw, flow_rev, npairs, h, w = _pair_flows(flow_fw, _f(flow_rev))
    frames, noc = _clip_frames(frames, npairs + 1, h, w)
    masks = [_mask(m, (npairs, h, w)) for m in (mask_fw, mask_rev)]
    with DeviceCall() as c:
        check(lib().ofdis_temporal_filter(*[c.input(x) for x in (frames, flow_fw, flow_rev, *masks)],
                                          c.output(frames.shape, np.uint8), c.output((npairs + 1, h, w), np.uint8, support),
                                          npairs, w, h, noc, wn, tau, None))
        return c.results()


def _weights(weights):
    w = np.ascontiguousarray(np.atleast_1d(np.asarray(weights, _f32)).ravel())
    return w, w.ctypes.data


def trajectory_filter(frames, flow_fw, flow_rev, weights, tau=np.inf, fb_check=True, alpha=FB_ALPHA, beta=FB_BETA, support=True):
    """ofdis_trajectory_filter on the device: frames uint8 [npairs + 1, h, w] (gray) or [npairs + 1, h, w, 3]; flow_fw / flow_rev
    [npairs, h, w, 2] float32 (frame k -> k + 1 and frame k + 1 -> k); weights: a sequence of 1..TRAJ_MAX_RADIUS values in
    [0, 1], its length is the radius.  Returns (out, the shape of frames; support uint8 [npairs + 1, h, w] = nf | nb << 4, or
    None with support=False: passed as NULL).  of_dis_amd/temporal.py: trajectory_filter_ref is the numpy statement of the same
    arithmetic, trajectory_weights makes the weights and reach splits the support."""
    flow_fw, flow_rev, npairs, h, w = _pair_flows(flow_fw, _f(flow_rev))
    frames, noc = _clip_frames(frames, npairs + 1, h, w)
    wts, wp = _weights(weights)
    with DeviceCall() as c:
        check(lib().ofdis_trajectory_filter(c.input(frames), c.input(flow_fw), c.input(flow_rev), c.output(frames.shape, np.uint8),
                                            c.output((npairs + 1, h, w), np.uint8, support), npairs, w, h, noc, wp, wts.size,
                                            tau, int(fb_check), alpha, beta, None))
        return c.results()


def _gm_inputs(flow, mask):
    """(flow [npairs, h, w, 2] float32, its optional mask uint8 [npairs, h, w], npairs, h, w)"""
    flow, _, npairs, h, w = _pair_flows(flow)
    return flow, _mask(mask, (npairs, h, w)), npairs, h, w


# The camera-model families by nparam, the doubles per model (a pair's model takes nparam * 8 bytes): the C functions of the
# fit (its work buffer: <fit>_work_bytes) and of the compensation, standalone and batch.  Only the 6-parameter fits take `model`.
_CAMERA = {6: dict(fit="ofdis_global_motion", compensate="ofdis_motion_compensate", batch_fit="ofdis_batch_global_motion",
                   batch_compensate="ofdis_batch_motion_compensate", model_arg=True),
           8: dict(fit="ofdis_projective_motion", compensate="ofdis_projective_compensate",
                   batch_fit="ofdis_batch_projective_motion", batch_compensate="ofdis_batch_projective_compensate",
                   model_arg=False)}


def _camera_fit(nparam, flow, mask, model, rounds, thresh, stats):
    fam = _CAMERA[nparam]
    flow, mask, npairs, h, w = _gm_inputs(flow, mask)
    wb = getattr(lib(), fam["fit"] + "_work_bytes")(npairs, w, h)
    fit = getattr(lib(), fam["fit"])
    with DeviceCall() as c:
        check(fit(c.input(flow), c.input(mask), npairs, w, h, *([model] if fam["model_arg"] else []), rounds, thresh,
                  c.output((npairs, nparam), np.float64), c.output((npairs, 3), np.int64, stats), c.work(wb), wb, None))
        return c.results()


def _camera_compensate(nparam, flow, models, mask, thresh, residual, label, in_place):
    flow, mask, npairs, h, w = _gm_inputs(flow, mask)
    models = np.ascontiguousarray(models, np.float64)
    assert models.shape == (npairs, nparam), models.shape
    compensate = getattr(lib(), _CAMERA[nparam]["compensate"])
    with DeviceCall() as c:
        pflow = c.input(flow)
        check(compensate(pflow, c.input(mask), c.input(models), npairs, w, h, thresh,
                         c.output(flow.shape, _f32, residual, over=pflow if in_place else None),
                         c.output((npairs, h, w), np.uint8, label), None))
        return c.results()


def global_motion(flow, mask=None, model=GM_AFFINE, rounds=3, thresh=1.0, stats=True):
    """ofdis_global_motion on the device: flow [npairs, h, w, 2] float32, mask uint8 [npairs, h, w] or None (all consistent)
    -> (models [npairs, 6] float64, stats [npairs, 3] int64: |S_0|, the size of the last set used, the status; None with
    stats=False, which passes NULL).  of_dis_amd/gmotion.py: global_motion_ref is the numpy statement of the same arithmetic."""
    return _camera_fit(6, flow, mask, model, rounds, thresh, stats)


def motion_compensate(flow, models, mask=None, thresh=1.0, residual=True, label=True, in_place=False):
    """ofdis_motion_compensate on the device: flow [npairs, h, w, 2] float32, models [npairs, 6] float64, mask as above ->
    (residual [npairs, h, w, 2] float32, label [npairs, h, w] uint8); residual=False / label=False pass NULL and return None in
    that place.  in_place: `residual` is the flow's own device array (the library allows it)."""
    return _camera_compensate(6, flow, models, mask, thresh, residual, label, in_place)


def projective_motion(flow, mask=None, rounds=3, thresh=1.0, stats=True):
    """ofdis_projective_motion on the device: flow and mask as global_motion takes them -> (models [npairs, 8] float64, stats
    [npairs, 3] int64: |S_0|, the size of the last set used, the parameters solved: 8, 6, 2 or 0; None with stats=False, which
    passes NULL).  of_dis_amd/gmotion.py: projective_motion_ref is the numpy statement of the same arithmetic."""
    return _camera_fit(8, flow, mask, None, rounds, thresh, stats)


def projective_compensate(flow, models, mask=None, thresh=1.0, residual=True, label=True, in_place=False):
    """ofdis_projective_compensate on the device: motion_compensate with models [npairs, 8] float64."""
    return _camera_compensate(8, flow, models, mask, thresh, residual, label, in_place)


def label_segments(label, flow=None, codes=SEG_MOVING, conn=8, min_area=0, max_segments=None, segments=True, records=True,
                   records_fill=None):
    """ofdis_label_segments on the device: label uint8 [nmaps, h, w], flow float32 [nmaps, h, w, 2] or None ->
    (segments int32 [nmaps, h, w], records int64 [nmaps, max_segments, 12], info int64 [nmaps, 4]: ncomp, nkept,
    min(nkept, max_segments), foreground pixels); segments=False / records=False pass NULL and return None in that place.
    max_segments None: one slot per pixel (never truncates).  Only the record slots < info[:, 2] are written: the others keep
    records_fill (int64, the records' shape), or zeros.  of_dis_amd/segments.py: label_segments_ref is the definition in numpy."""
    label = np.ascontiguousarray(label, np.uint8)
    assert label.ndim == 3, label.shape
    nmaps, h, w = label.shape
    if max_segments is None:
        max_segments = min(h * w, SEG_MAX_SEGMENTS)
    if flow is not None:
        flow = _f(flow)
        assert flow.shape == (nmaps, h, w, 2), flow.shape
    rshape = (nmaps, max_segments, SEG_RECORD_FIELDS)
    if records and records_fill is None:
        records_fill = np.zeros(rshape, np.int64)
    wb = lib().ofdis_segments_work_bytes(nmaps, w, h)
    with DeviceCall() as c:
        check(lib().ofdis_label_segments(c.input(label), c.input(flow), nmaps, w, h, codes, conn, min_area, max_segments,
                                         c.output((nmaps, h, w), np.int32, segments),
                                         c.output(rshape, np.int64, records, fill=records_fill),
                                         c.output((nmaps, SEG_INFO_FIELDS), np.int64), c.work(wb), wb, None))
        return c.results()


def segment_tracks_work_bytes(nmaps, max_segments):
    """ofdis_segment_tracks_work_bytes: the work buffer of segment_tracks; 0 for rejected arguments."""
    return lib().ofdis_segment_tracks_work_bytes(nmaps, max_segments)


def _st_maps(segments, info):
    """segments int32 [nmaps, h, w] and info int64 [nmaps, 4] of label_segments: (segments, info, nmaps, h, w)"""
    segments, info = np.ascontiguousarray(segments, np.int32), np.ascontiguousarray(info, np.int64)
    assert segments.ndim == 3 and info.shape == (segments.shape[0], SEG_INFO_FIELDS), (segments.shape, info.shape)
    return (segments, info) + segments.shape


def _st_array(a, dtype, shape):
    """an input of `shape`; one of no elements (a clip of one map has no pair) is uploaded as 8 bytes that are never read"""
    a = np.ascontiguousarray(a, dtype).reshape(shape)
    return a if a.size else np.zeros(8 // np.dtype(dtype).itemsize, dtype)


def _st_output(c, shape, dtype, fill):
    """an output that starts from `fill` (None: zeros): the slots a definition leaves alone keep it"""
    if not int(np.prod(shape)):
        return c.output(shape, dtype)
    return c.output(shape, dtype, fill=np.zeros(shape, dtype) if fill is None else fill)


def segment_overlap(segments, flow, info, max_segments, overlap_fill=None):
    """ofdis_segment_overlap on the device: segments int32 [nmaps, h, w] and info int64 [nmaps, 4] as label_segments returns
    them, flow float32 [nmaps, h, w, 2] taking frame k to k + 1 -> overlap int32 [nmaps - 1, S, S].  Only [k, :n_k, :n_{k+1}]
    is written: the rest keeps overlap_fill (int32, that shape), or zeros.  segments.py: segment_overlap_ref."""
    segments, info, nmaps, h, w = _st_maps(segments, info)
    flow = _f(flow)
    assert flow.shape == (nmaps, h, w, 2), flow.shape
    S = max_segments
    with DeviceCall() as c:
        check(lib().ofdis_segment_overlap(c.input(segments), c.input(flow), c.input(info), nmaps, w, h, S,
                                          _st_output(c, (nmaps - 1, S, S), np.int32, overlap_fill), None))
        return c.results()[0]


def segment_link(overlap, records, info, max_segments, min_share, link_fill=None):
    """ofdis_segment_link on the device: overlap int32 [nmaps - 1, S, S], records int64 [nmaps, S, 12], info int64 [nmaps, 4]
    -> link int32 [nmaps - 1, S]; only [k, :n_k] is written: the rest keeps link_fill, or zeros.  segments.py: segment_link_ref."""
    info = np.ascontiguousarray(info, np.int64)
    nmaps, S = len(info), max_segments
    with DeviceCall() as c:
        check(lib().ofdis_segment_link(c.input(_st_array(overlap, np.int32, (nmaps - 1, S, S))),
                                       c.input(_st_array(records, np.int64, (nmaps, S, SEG_RECORD_FIELDS))), c.input(info), nmaps, S,
                                       min_share, _st_output(c, (nmaps - 1, S), np.int32, link_fill), None))
        return c.results()[0]


def segment_chain(link, records, info, max_segments, max_tracks, ids_fill=None, tracks_fill=None):
    """ofdis_segment_chain on the device: link int32 [nmaps - 1, S], records, info -> (ids int32 [nmaps, S], tracks int64
    [max_tracks, 12], tinfo int64 [4] = ntracks, tracks written, links followed, longest length).  ids [k, :n_k] and the first
    tinfo[1] track records are written: the rest keeps ids_fill / tracks_fill, or zeros.  segments.py: segment_chain_ref."""
    info = np.ascontiguousarray(info, np.int64)
    nmaps, S = len(info), max_segments
    with DeviceCall() as c:
        check(lib().ofdis_segment_chain(c.input(_st_array(link, np.int32, (nmaps - 1, S))),
                                        c.input(_st_array(records, np.int64, (nmaps, S, SEG_RECORD_FIELDS))), c.input(info), nmaps, S,
                                        max_tracks, _st_output(c, (nmaps, S), np.int32, ids_fill),
                                        _st_output(c, (max_tracks, SEGTRACK_FIELDS), np.int64, tracks_fill),
                                        c.output((SEGTRACK_INFO_FIELDS,), np.int64), None))
        return c.results()


def segment_relabel(segments, ids, info, max_segments, track_map_fill=None):
    """ofdis_segment_relabel on the device: segments int32 [nmaps, h, w], ids int32 [nmaps, S], info -> track_map int32
    [nmaps, h, w].  Every entry is written: nothing of track_map_fill (the array it starts from) stays.  segments.py:
    segment_relabel_ref."""
    segments, info, nmaps, h, w = _st_maps(segments, info)
    S = max_segments
    with DeviceCall() as c:
        check(lib().ofdis_segment_relabel(c.input(segments), c.input(_st_array(ids, np.int32, (nmaps, S))), c.input(info), nmaps, w, h,
                                          S, _st_output(c, (nmaps, h, w), np.int32, track_map_fill), None))
        return c.results()[0]


def segment_tracks(segments, flow, records, info, max_segments, min_share=50, max_tracks=None, track_map=True, ids_fill=None,
                   tracks_fill=None, track_map_fill=None):
    """ofdis_segment_tracks on the device, the four steps in one call: (segments, records, info) of label_segments called with
    max_segments, flow float32 [nmaps, h, w, 2] taking frame k to k + 1 -> (ids int32 [nmaps, S], tracks int64 [max_tracks, 12],
    tinfo int64 [4], track_map int32 [nmaps, h, w] or None with track_map=False, which passes NULL).  max_tracks None: a slot
    for every segment.  The fills as in segment_chain and segment_relabel.  segments.py: segment_tracks_ref."""
    segments, info, nmaps, h, w = _st_maps(segments, info)
    flow = _f(flow)
    assert flow.shape == (nmaps, h, w, 2), flow.shape
    S = max_segments
    if max_tracks is None:
        max_tracks = min(nmaps * S, SEGTRACK_MAX_TRACKS)
    wb = segment_tracks_work_bytes(nmaps, S)
    with DeviceCall() as c:
        check(lib().ofdis_segment_tracks(c.input(segments), c.input(flow), c.input(_st_array(records, np.int64, (nmaps, S, SEG_RECORD_FIELDS))),
                                         c.input(info), nmaps, w, h, S, min_share, max_tracks,
                                         _st_output(c, (nmaps, S), np.int32, ids_fill),
                                         _st_output(c, (max_tracks, SEGTRACK_FIELDS), np.int64, tracks_fill),
                                         c.output((SEGTRACK_INFO_FIELDS,), np.int64),
                                         _st_output(c, (nmaps, h, w), np.int32, track_map_fill) if track_map else c.output((nmaps, h, w), np.int32, False),
                                         c.work(wb), wb, None))
        return c.results()


def _stab_weights(weights):
    """the window as a host array of radius + 1 doubles: (array, radius)"""
    weights = np.ascontiguousarray(weights, np.float64)
    assert weights.ndim == 1 and weights.size >= 1, weights.shape
    return weights, weights.size - 1


def camera_path(models, weights, zoom=1.0):
    """ofdis_camera_path on the device: models [npairs, 6] float64 (global_motion's), weights [radius + 1] float64 (host; e.g.
    of_dis_amd.stabilize.gaussian_weights) -> warps [npairs + 1, 6] float64, one per frame.
    of_dis_amd/stabilize.py: camera_path_ref is the numpy statement of the same arithmetic."""
    models = np.ascontiguousarray(models, np.float64)
    assert models.ndim == 2 and models.shape[1] == 6, models.shape
    npairs = models.shape[0]
    weights, radius = _stab_weights(weights)
    with DeviceCall() as c:
        check(lib().ofdis_camera_path(c.input(models), npairs, weights.ctypes.data, radius, zoom,
                                      c.output((npairs + 1, 6), np.float64), None))
        return c.results()[0]


def warp_frames(frames, warps, border=BORDER_CONSTANT, inside=True):
    """ofdis_warp_frames on the device: frames uint8 [n, h, w] (gray) or [n, h, w, 3], warps [n, 6] float64 -> (out, the shape
    of frames; inside uint8 [n, h, w], or None with inside=False: passed as NULL).
    of_dis_amd/stabilize.py: warp_frames_ref is the numpy statement of the same arithmetic."""
    n, h, w = np.shape(frames)[:3]
    frames, noc = _clip_frames(frames, n, h, w)
    warps = np.ascontiguousarray(warps, np.float64)
    assert warps.shape == (n, 6), warps.shape
    with DeviceCall() as c:
        check(lib().ofdis_warp_frames(c.input(frames), c.input(warps), c.output(frames.shape, np.uint8),
                                      c.output((n, h, w), np.uint8, inside), n, w, h, noc, border, None))
        return c.results()


def camera_path_projective(models, weights, w, h, zoom=1.0):
    """ofdis_camera_path_projective on the device: models [npairs, 8] float64 (projective_motion's) of a clip of w x h frames,
    weights as camera_path takes them -> warps [npairs + 1, 8] float64, one per frame.
    of_dis_amd/stabilize.py: camera_path_projective_ref is the numpy statement of the same arithmetic."""
    models = np.ascontiguousarray(models, np.float64)
    assert models.ndim == 2 and models.shape[1] == 8, models.shape
    npairs = models.shape[0]
    weights, radius = _stab_weights(weights)
    with DeviceCall() as c:
        check(lib().ofdis_camera_path_projective(c.input(models), npairs, w, h, weights.ctypes.data, radius, zoom,
                                                 c.output((npairs + 1, 8), np.float64), None))
        return c.results()[0]


def warp_frames_projective(frames, warps, border=BORDER_CONSTANT, inside=True):
    """ofdis_warp_frames_projective on the device: warp_frames with warps [n, 8] float64.
    of_dis_amd/stabilize.py: warp_frames_projective_ref is the numpy statement of the same arithmetic."""
    n, h, w = np.shape(frames)[:3]
    frames, noc = _clip_frames(frames, n, h, w)
    warps = np.ascontiguousarray(warps, np.float64)
    assert warps.shape == (n, 8), warps.shape
    with DeviceCall() as c:
        check(lib().ofdis_warp_frames_projective(c.input(frames), c.input(warps), c.output(frames.shape, np.uint8),
                                                 c.output((n, h, w), np.uint8, inside), n, w, h, noc, border, None))
        return c.results()


class Batch:
    """ofdis_batch: `nframes` frame pairs of one geometry resident in HBM.  reverse=True: ofdis_batch_create_ex with
    OFDIS_BATCH_REVERSE (every pass also computes the flow B -> A of each pair).  stereo_lr=True: OFDIS_BATCH_STEREO_LR
    (stereo-depth mode: every pass also runs on the mirrored, swapped pair, which gives the right view's disparity).
    sequence=True: OFDIS_BATCH_SEQUENCE (nframes + 1 consecutive frames, each held once; pair k = frames k, k + 1; filled
    through build_pyramids_u8_seq or upload_frame)."""

    def __init__(self, p, nframes, reverse=False, stereo_lr=False, sequence=False):
        self.p = p.copy()
        self.nframes = nframes
        self.reverse = bool(reverse)
        self.stereo_lr = bool(stereo_lr)
        self.sequence = bool(sequence)
        self.h = VP()
        flags = ((BATCH_REVERSE if reverse else 0) | (BATCH_STEREO_LR if stereo_lr else 0) |
                 (BATCH_SEQUENCE if sequence else 0))
        check(lib().ofdis_batch_create_ex(C.byref(self.h), C.byref(self.p), nframes, flags))

    def close(self):
        if self.h:
            lib().ofdis_batch_destroy(self.h)
            self.h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def input_ptr(self, level, kind):
        return lib().ofdis_batch_input(self.h, level, kind)

    def input_elems(self, level):
        return lib().ofdis_batch_input_elems(self.h, level)

    def input_frames(self):
        """ofdis_batch_input_frames: frame slots of the input arrays (nframes + 1 for a sequence context)."""
        return lib().ofdis_batch_input_frames(self.h)

    def device_bytes(self):
        """ofdis_batch_device_bytes: bytes of device memory in the arrays the context holds right now."""
        return lib().ofdis_batch_device_bytes(self.h)

    def upload_frame(self, slot, pyr, pyr_dx, pyr_dy, stream=None):
        """ofdis_batch_upload_frame: one frame's host pyramid (lists over levels 0..sc_f) into frame slot 0..nframes."""
        n = self.p.sc_f + 1
        keep = [[_f(x) if x is not None else None for x in pl] for pl in (pyr, pyr_dx, pyr_dy)]
        check(lib().ofdis_batch_upload_frame(self.h, slot, _ptr_array(keep[0], n), _ptr_array(keep[1], n),
                                             _ptr_array(keep[2], n), stream))
        check(lib().ofdis_sync(stream))

    def upload(self, frame, pyr_a, pyr_a_dx, pyr_a_dy, pyr_b, stream=None):
        n = self.p.sc_f + 1
        keep = [[_f(x) if x is not None else None for x in pl] for pl in (pyr_a, pyr_a_dx, pyr_a_dy, pyr_b)]
        check(lib().ofdis_batch_upload(self.h, frame, _ptr_array(keep[0], n), _ptr_array(keep[1], n),
                                       _ptr_array(keep[2], n), _ptr_array(keep[3], n), stream))
        check(lib().ofdis_sync(stream))

    def upload_b_gradients(self, frame, pyr_b_dx, pyr_b_dy, stream=None):
        n = self.p.sc_f + 1
        keep = [[_f(x) if x is not None else None for x in pl] for pl in (pyr_b_dx, pyr_b_dy)]
        check(lib().ofdis_batch_upload_b_gradients(self.h, frame, _ptr_array(keep[0], n), _ptr_array(keep[1], n), stream))
        check(lib().ofdis_sync(stream))

    def set_input(self, level, kind, arr):
        """arr: [nframes, tmp_h, tmp_w, noc] float32 host array"""
        arr = _f(arr)
        assert arr.size == self.input_elems(level) * self.nframes, (arr.shape, self.input_elems(level))
        check(lib().ofdis_memcpy_h2d(self.input_ptr(level, kind), arr.ctypes.data, arr.nbytes))

    def upload_initflow(self, frame, initflow, stream=None):
        a = _f(initflow)
        assert a.size == lib().ofdis_batch_initflow_elems(self.h), (a.shape, lib().ofdis_batch_initflow_elems(self.h))
        check(lib().ofdis_batch_upload_initflow(self.h, frame, a.ctypes.data_as(FP), stream))
        check(lib().ofdis_sync(stream))  # `a` may be a temporary: the copy must have read it before it goes away

    def set_initflow(self, dev_ptr):
        check(lib().ofdis_batch_set_initflow(self.h, dev_ptr))

    def build_pyramids_u8(self, img_a_ptr, img_b_ptr, width_org, height_org, stream=None):
        check(lib().ofdis_batch_build_pyramids_u8(self.h, img_a_ptr, img_b_ptr, width_org, height_org, stream))

    def build_pyramids_u8_seq(self, frames_ptr, width_org, height_org, row_pitch=0, frame_stride=0, stream=None):
        """ofdis_batch_build_pyramids_u8_seq: frames_ptr = device pointer to nframes + 1 frames, row y of frame f at
        frames_ptr + f * frame_stride + y * row_pitch (0, 0: packed)."""
        check(lib().ofdis_batch_build_pyramids_u8_seq(self.h, frames_ptr, row_pitch, frame_stride, width_org, height_org, stream))

    def run(self, stream=None):
        check(lib().ofdis_batch_run(self.h, stream))

    def set_pipeline(self, sub_batches):
        check(lib().ofdis_batch_set_pipeline(self.h, sub_batches))

    def set_graph(self, mode):
        check(lib().ofdis_batch_set_graph(self.h, mode))

    def join(self, stream=None):
        check(lib().ofdis_batch_join(self.h, stream))

    def status(self):
        """ofdis_batch_status: 0, or OFDIS_ERR_DEVICE (-3) when the last pass's results are invalid (call after a sync)."""
        return lib().ofdis_batch_status(self.h)

    def flow_ptr(self):
        return lib().ofdis_batch_flow(self.h)

    def download(self, frame, stream=None):
        w, h = self.p.level_size(self.p.sc_l)
        out = np.zeros((h, w, self.p.nop), _f32)
        check(lib().ofdis_batch_download(self.h, frame, out.ctypes.data_as(FP), stream))
        return out

    def upsample(self, width_org, height_org, out_ptr=None, stream=None):
        """ofdis_batch_upsample.  With out_ptr (device pointer) only enqueues; otherwise returns the host array
        [nframes][height_org][width_org][2]."""
        shape = (self.nframes, height_org, width_org, self.p.nop)
        with DeviceCall(stream, own=out_ptr is None) as c:
            check(lib().ofdis_batch_upsample(self.h, c.output(shape, _f32, out_ptr or True), width_org, height_org, stream))
            res = c.results()
        return res[0] if res else None

    def upsample_frames(self, first, count, width_org, height_org, stream=None):
        """ofdis_batch_upsample_frames: the full-resolution flow of frames [first, first + count) as a host array."""
        with DeviceCall(stream) as c:
            check(lib().ofdis_batch_upsample_frames(self.h, first, count, c.output((count, height_org, width_org, self.p.nop)),
                                                    width_org, height_org, stream))
            return c.results()[0]

    def upsample_frames_enc(self, first, count, width_org, height_org, enc, stream=None):
        """ofdis_batch_upsample_frames_enc: the full-resolution result of frames [first, first + count) written in the
        encoding `enc` (an Encoding), as a host array [count][height_org][width_org][nop] of enc.dtype."""
        shape = (count, height_org, width_org, self.p.nop)
        with DeviceCall(stream) as c:
            check(lib().ofdis_batch_upsample_frames_enc(self.h, first, count, c.output(shape, _enc_dtype(enc)), width_org,
                                                        height_org, C.byref(enc), stream))
            return c.results()[0]

    def _flow_array(self, ptr, level, missing=None):
        """A level's flow array at device pointer `ptr` as a host array [nframes][h][w][nop], the pass joined first.  `missing`:
        what a null `ptr` means."""
        if missing and not ptr:
            raise OfdisError(missing)
        w, h = self.p.level_size(level)
        out = np.zeros((self.nframes, h, w, self.p.nop), _f32)
        self.join(None)
        check(lib().ofdis_sync(None))
        check(lib().ofdis_memcpy_d2h(out.ctypes.data, ptr, out.nbytes))
        return out

    def download_all(self):
        return self._flow_array(self.flow_ptr(), self.p.sc_l)

    def level_flow(self, level):
        return self._flow_array(lib().ofdis_batch_level_flow(self.h, level), level)

    # ---- reverse direction (reverse=True contexts)
    def set_initflow_reverse(self, dev_ptr):
        check(lib().ofdis_batch_set_initflow_reverse(self.h, dev_ptr))

    def download_reverse(self, frame, stream=None):
        w, h = self.p.level_size(self.p.sc_l)
        out = np.zeros((h, w, self.p.nop), _f32)
        check(lib().ofdis_batch_download_reverse(self.h, frame, out.ctypes.data_as(FP), stream))
        return out

    def level_flow_reverse(self, level):
        return self._flow_array(lib().ofdis_batch_level_flow_reverse(self.h, level), level,
                                "ofdis_batch_level_flow_reverse: not a reverse context, or no such level")

    def download_all_reverse(self):
        return self.level_flow_reverse(self.p.sc_l)

    # ---- stereo left-right (stereo_lr=True contexts)
    def level_flow_mirror(self, level):
        """The raw mirror-pass disparity of a level (mirrored coordinates, <= 0): for the parity tests."""
        return self._flow_array(lib().ofdis_batch_level_flow_mirror(self.h, level), level,
                                "ofdis_batch_level_flow_mirror: not a stereo_lr context, or no such level")

    def upsample_lr(self, width_org, height_org, fill=FILL_NONE, alpha=FB_ALPHA, beta=FB_BETA, first=0, count=None,
                    outputs=(True, True, True, True), stream=None):
        """ofdis_batch_upsample_lr over frames [first, first + count): (left, right, mask_left, mask_right) as host arrays
        [count][height_org][width_org], float32 and uint8.  `outputs` selects which of the four the library writes (the
        others are passed as NULL and returned as None)."""
        count = self.nframes - first if count is None else count
        shape = (count, height_org, width_org)
        with DeviceCall(stream) as c:
            ptrs = [c.output(shape, t, want) for want, t in zip(outputs, (_f32, _f32, np.uint8, np.uint8))]
            check(lib().ofdis_batch_upsample_lr(self.h, first, count, *ptrs, fill, width_org, height_org, alpha, beta, stream))
            return c.results()

    def upsample_bidir(self, width_org, height_org, alpha=FB_ALPHA, beta=FB_BETA, first=0, count=None,
                       outputs=(True, True, True, True), stream=None):
        """ofdis_batch_upsample_bidir over frames [first, first + count): (fw, rev, mask_fw, mask_rev) as host arrays,
        [count][height_org][width_org][2] float32 and [count][height_org][width_org] uint8.  `outputs` selects which of the
        four the library writes (the others are passed as NULL and returned as None)."""
        count = self.nframes - first if count is None else count
        shapes = [(count, height_org, width_org, 2)] * 2 + [(count, height_org, width_org)] * 2
        with DeviceCall(stream) as c:
            ptrs = [c.output(shape, t, want) for want, shape, t in zip(outputs, shapes, (_f32, _f32, np.uint8, np.uint8))]
            check(lib().ofdis_batch_upsample_bidir(self.h, first, count, *ptrs, width_org, height_org, alpha, beta, stream))
            return c.results()

    def interpolate(self, img_a_ptr, img_b_ptr, width_org, height_org, times, first=0, count=None, alpha=FB_ALPHA,
                    beta=FB_BETA, out_ptr=None, stream=None):
        """ofdis_batch_interpolate over frames [first, first + count): img_a_ptr / img_b_ptr are the whole device arrays given
        to build_pyramids_u8.  out_ptr None: returns the host array [count][len(times)][height_org][width_org] (+ [noc]
        for RGB); else writes the device array out_ptr on `stream` and returns None."""
        count = self.nframes - first if count is None else count
        t, tp = _times(times)
        shape = (count, t.size, height_org, width_org) + ((self.p.noc,) if self.p.noc > 1 else ())
        with DeviceCall(stream, own=out_ptr is None) as c:
            check(lib().ofdis_batch_interpolate(self.h, img_a_ptr, img_b_ptr, first, count, tp, t.size,
                                                c.output(shape, np.uint8, out_ptr or True), width_org, height_org, alpha, beta,
                                                stream))
            res = c.results()
        return res[0] if res else None

    def track_points(self, seeds, width_org, height_org, seed_frame=None, max_steps=0, fb_check=True, first=0, count=None,
                     alpha=FB_ALPHA, beta=FB_BETA, stream=None):
        """ofdis_batch_track_points over the pairs [first, first + count) of a sequence=True context, straight from its level
        flows: seeds [npoints, 2] float32, seed_frame [npoints] int32 relative to `first` or None -> (tracks [count + 1,
        npoints, 2] float32, counts [npoints] int32).  fb_check=True needs reverse=True."""
        count = self.nframes - first if count is None else count
        seeds, seed_frame = _track_inputs(seeds, seed_frame)
        n = seeds.shape[0]
        with DeviceCall(stream) as c:
            check(lib().ofdis_batch_track_points(self.h, first, count, c.input(seeds), c.input(seed_frame), n, max_steps,
                                                 int(fb_check), alpha, beta, c.output((count + 1, n, 2)), c.output((n,), np.int32),
                                                 width_org, height_org, stream))
            return c.results()

    def dense_tracks(self, frames_ptr, width_org, height_org, stride, window, min_eig, max_len=15, fb_check=True,
                     max_tracks=None, first=0, count=None, alpha=FB_ALPHA, beta=FB_BETA, stream=None):
        """ofdis_batch_dense_tracks over the pairs [first, first + count) of a sequence=True context, straight from its level
        flows: frames_ptr is the whole packed device clip given to build_pyramids_u8_seq.  Returns what capi.dense_tracks
        returns, `start` relative to `first`.  fb_check=True needs reverse=True; max_tracks None: room for every seed."""
        count = self.nframes - first if count is None else count
        ncx, ncy = dense_tracks_cells(width_org, height_org, stride)
        if max_tracks is None:
            max_tracks = max(1, min(max(count, 1) * ncx * ncy, DT_MAX_TRACKS))
        lmax = _dense_lmax(max_len, max(count, 1))
        with DeviceCall(stream) as c:
            check(lib().ofdis_batch_dense_tracks(self.h, frames_ptr, first, count, stride, window, min_eig, max_len, int(fb_check),
                                                 alpha, beta, max_tracks,
                                                 *_dense_declare(c, lmax, max(1, min(max_tracks, DT_MAX_TRACKS))), width_org,
                                                 height_org, stream))
            return _dense_cut(c.results(), lmax, max_tracks)

    def temporal_filter(self, frames_ptr, width_org, height_org, wn=1.0, tau=np.inf, first=0, count=None, alpha=FB_ALPHA,
                        beta=FB_BETA, out_ptr=None, support=False, stream=None):
        """ofdis_batch_temporal_filter over the frames first .. first + count of a sequence=True, reverse=True context, straight
        from its level flows: frames_ptr is the whole packed device clip given to build_pyramids_u8_seq.  out_ptr None: returns
        the host array [count + 1][height_org][width_org] (+ [noc] for RGB), with support=True the pair (out, support
        [count + 1][height_org][width_org]); else writes the device array out_ptr (and, if `support` is a device pointer, that
        array) on `stream` and returns None."""
        count = self.nframes - first if count is None else count
        shape = (max(count, 0) + 1, height_org, width_org)
        oshape = shape + ((self.p.noc,) if self.p.noc > 1 else ())
        with DeviceCall(stream, own=out_ptr is None) as c:
            check(lib().ofdis_batch_temporal_filter(self.h, frames_ptr, first, count, c.output(oshape, np.uint8, out_ptr or True),
                                                    c.output(shape, np.uint8, support), width_org, height_org, wn, tau, alpha, beta,
                                                    stream))
            res = c.results()
        return res if res is None or support else res[0]

    def trajectory_filter(self, frames_ptr, width_org, height_org, weights, tau=np.inf, fb_check=True, first=0, count=None,
                          alpha=FB_ALPHA, beta=FB_BETA, out_ptr=None, support=False, stream=None):
        """ofdis_batch_trajectory_filter over the frames first .. first + count of a sequence=True, reverse=True context,
        straight from its level flows: frames_ptr is the whole packed device clip given to build_pyramids_u8_seq; weights: a
        sequence of 1..TRAJ_MAX_RADIUS values in [0, 1], its length is the radius.  Returns and writes what temporal_filter
        does: out_ptr None: the host array [count + 1][height_org][width_org] (+ [noc] for RGB), with support=True the pair
        (out, support [count + 1][height_org][width_org] = nf | nb << 4); else the device array out_ptr (and, if `support` is a
        device pointer, that array) on `stream`, and None."""
        count = self.nframes - first if count is None else count
        shape = (max(count, 0) + 1, height_org, width_org)
        oshape = shape + ((self.p.noc,) if self.p.noc > 1 else ())
        wts, wp = _weights(weights)
        with DeviceCall(stream, own=out_ptr is None) as c:
            check(lib().ofdis_batch_trajectory_filter(self.h, frames_ptr, first, count, c.output(oshape, np.uint8, out_ptr or True),
                                                      c.output(shape, np.uint8, support), width_org, height_org, wp, wts.size, tau,
                                                      int(fb_check), alpha, beta, stream))
            res = c.results()
        return res if res is None or support else res[0]

    def _camera_fit(self, nparam, width_org, height_org, model, rounds, thresh, fb_check, first, count, alpha, beta, models_ptr,
                    stats_ptr, stream):
        fam = _CAMERA[nparam]
        count = self.nframes - first if count is None else count
        fit = getattr(lib(), fam["batch_fit"])
        own = models_ptr is None  # (then both arrays are the call's own: stats_ptr counts only beside models_ptr)
        with DeviceCall(stream, own) as c:
            check(fit(self.h, first, count, *([model] if fam["model_arg"] else []), rounds, thresh, int(fb_check), alpha, beta,
                      c.output((count, nparam), np.float64, own or models_ptr), c.output((count, 3), np.int64, own or stats_ptr),
                      width_org, height_org, stream))
            return c.results()

    def _camera_compensate(self, nparam, models, width_org, height_org, thresh, fb_check, first, count, alpha, beta, residual,
                           label, out_ptr, stream):
        count = self.nframes - first if count is None else count
        n = max(count, 1)
        on_host = not isinstance(models, (int, type(None)))
        if on_host:
            models = np.ascontiguousarray(models, np.float64)
            assert models.shape == (n, nparam), models.shape
        rshape, lshape = (n, height_org, width_org, 2), (n, height_org, width_org)
        want_r, want_l = (residual, label) if out_ptr is None else out_ptr
        compensate = getattr(lib(), _CAMERA[nparam]["batch_compensate"])
        with DeviceCall(stream, own=out_ptr is None) as c:  # (uploaded models outlive the launch: results() synchronises for them)
            check(compensate(self.h, first, count, c.input(models) if on_host else models, thresh, int(fb_check), alpha, beta,
                             c.output(rshape, _f32, want_r), c.output(lshape, np.uint8, want_l), width_org, height_org, stream))
            return c.results()

    def global_motion(self, width_org, height_org, model=GM_AFFINE, rounds=3, thresh=1.0, fb_check=False, first=0, count=None,
                      alpha=FB_ALPHA, beta=FB_BETA, models_ptr=None, stats_ptr=None, stream=None):
        """ofdis_batch_global_motion over the pairs [first, first + count) of an optical-flow context, straight from its level
        flows.  fb_check=True (needs reverse=True) honours the forward mask of upsample_bidir.  models_ptr None: returns the
        host arrays (models [count, 6] float64, stats [count, 3] int64); else writes the device array models_ptr (and stats_ptr,
        if given) on `stream` and returns None."""
        return self._camera_fit(6, width_org, height_org, model, rounds, thresh, fb_check, first, count, alpha, beta, models_ptr,
                                stats_ptr, stream)

    def motion_compensate(self, models, width_org, height_org, thresh=1.0, fb_check=False, first=0, count=None, alpha=FB_ALPHA,
                          beta=FB_BETA, residual=True, label=True, out_ptr=None, stream=None):
        """ofdis_batch_motion_compensate over the pairs [first, first + count): models is a host array [count, 6] float64 or a
        device pointer.  out_ptr None: returns the host arrays (residual [count, height_org, width_org, 2] float32, label
        [count, height_org, width_org] uint8; None where residual=False / label=False); else out_ptr = (residual device pointer
        or None, label device pointer or None), written on `stream`, and the call returns None."""
        return self._camera_compensate(6, models, width_org, height_org, thresh, fb_check, first, count, alpha, beta, residual,
                                       label, out_ptr, stream)

    def projective_motion(self, width_org, height_org, rounds=3, thresh=1.0, fb_check=False, first=0, count=None, alpha=FB_ALPHA,
                          beta=FB_BETA, models_ptr=None, stats_ptr=None, stream=None):
        """ofdis_batch_projective_motion: global_motion with the 8-parameter model.  models_ptr None: returns the host arrays
        (models [count, 8] float64, stats [count, 3] int64); else writes the device arrays on `stream` and returns None."""
        return self._camera_fit(8, width_org, height_org, None, rounds, thresh, fb_check, first, count, alpha, beta, models_ptr,
                                stats_ptr, stream)

    def projective_compensate(self, models, width_org, height_org, thresh=1.0, fb_check=False, first=0, count=None,
                              alpha=FB_ALPHA, beta=FB_BETA, residual=True, label=True, out_ptr=None, stream=None):
        """ofdis_batch_projective_compensate: motion_compensate with models [count, 8] float64 (host array or device pointer);
        the outputs as there."""
        return self._camera_compensate(8, models, width_org, height_org, thresh, fb_check, first, count, alpha, beta, residual,
                                       label, out_ptr, stream)

    def stabilize(self, frames_ptr, width_org, height_org, weights, zoom=1.0, border=BORDER_CONSTANT, model=GM_AFFINE, rounds=3,
                  thresh=1.0, fb_check=False, first=0, count=None, alpha=FB_ALPHA, beta=FB_BETA, inside=False, out_ptr=None,
                  warps_ptr=None, stream=None):
        """ofdis_batch_stabilize over the frames first .. first + count of a sequence=True context: the models of
        global_motion(model, rounds, thresh, fb_check) smoothed over the window `weights` (host, radius + 1 doubles) and the
        frames warped.  frames_ptr is the whole packed device clip given to build_pyramids_u8_seq.  out_ptr None: returns (out
        [count + 1][height_org][width_org] (+ [noc] for RGB), inside [count + 1][height_org][width_org] or None with
        inside=False, warps [count + 1, 6] float64); else writes the device arrays out_ptr, `inside` (if a device pointer) and
        warps_ptr (if given) on `stream` and returns None."""
        count = self.nframes - first if count is None else count
        weights, radius = _stab_weights(weights)
        shape = (max(count, 0) + 1, height_org, width_org)
        oshape = shape + ((self.p.noc,) if self.p.noc > 1 else ())
        with DeviceCall(stream, own=out_ptr is None) as c:
            check(lib().ofdis_batch_stabilize(self.h, frames_ptr, first, count, model, rounds, thresh, int(fb_check), alpha, beta,
                                              weights.ctypes.data, radius, zoom, border,
                                              c.output(oshape, np.uint8, out_ptr or True), c.output(shape, np.uint8, inside),
                                              c.output((shape[0], 6), np.float64, warps_ptr or out_ptr is None),
                                              width_org, height_org, stream))
            return c.results()

    def stabilize_projective(self, frames_ptr, width_org, height_org, weights, zoom=1.0, border=BORDER_CONSTANT, rounds=3,
                             thresh=1.0, fb_check=False, first=0, count=None, alpha=FB_ALPHA, beta=FB_BETA, inside=False,
                             out_ptr=None, warps_ptr=None, stream=None):
        """ofdis_batch_stabilize_projective: stabilize under the 8-parameter models of projective_motion(rounds, thresh,
        fb_check), the path chained on homographies and the frames resampled by a perspective warp.  Arguments and returns as
        stabilize, without `model`; the warps are [count + 1, 8] float64."""
        count = self.nframes - first if count is None else count
        weights, radius = _stab_weights(weights)
        shape = (max(count, 0) + 1, height_org, width_org)
        oshape = shape + ((self.p.noc,) if self.p.noc > 1 else ())
        with DeviceCall(stream, own=out_ptr is None) as c:
            check(lib().ofdis_batch_stabilize_projective(self.h, frames_ptr, first, count, rounds, thresh, int(fb_check), alpha,
                                                         beta, weights.ctypes.data, radius, zoom, border,
                                                         c.output(oshape, np.uint8, out_ptr or True),
                                                         c.output(shape, np.uint8, inside),
                                                         c.output((shape[0], 8), np.float64, warps_ptr or out_ptr is None),
                                                         width_org, height_org, stream))
            return c.results()

    def timing(self, enable=True):
        check(lib().ofdis_batch_timing(self.h, int(enable)))

    def kernel_time(self, k):
        ms, n = C.c_double(0), C.c_long(0)
        check(lib().ofdis_batch_kernel_time(self.h, k, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_times(self, k, capacity=4096):
        """Per-launch milliseconds of a kernel class in launch order (a pass launches a class once per level, coarsest first)."""
        buf, n = (C.c_double * capacity)(), C.c_int(0)
        check(lib().ofdis_batch_kernel_times(self.h, k, buf, capacity, C.byref(n)))
        return [buf[i] for i in range(min(n.value, capacity))]
