"""CPU: the C-ABI library loads and exports every symbol include/ofdis.h declares; host-side parameter
logic (operating points, geometry) matches the reference's derivations.  No compute calls (no GPU here)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import abi
from of_dis_amd import build, capi, encoding, gmotion, stabilize, temporal, tracking
from of_dis_amd.abi import prototypes
from of_dis_amd.params import OfdisParams, auto_first_scale, oppoint, padded_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPES = prototypes()


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "ofdis.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ofdis_[a-z0-9_]+)\s*\(", src)))


def test_header_and_binding_agree():
    """the parser misses no declaration: this loose regex counts on its own.  The export list is made by the same parser, so a
    prototype it missed would vanish from the library and from the binding together."""
    assert _declared_functions() == sorted(PROTOTYPES) == sorted(capi.ABI_SYMBOLS) == build.abi_symbols()
    assert len(PROTOTYPES) == len(capi.ABI_SYMBOLS)


@pytest.mark.parametrize("name", PROTOTYPES)
def test_declared_bound_and_exported(name):
    fn = getattr(capi.lib(), name)
    assert fn.argtypes is not None and (fn.restype, list(fn.argtypes)) == PROTOTYPES[name]
    assert name in abi.exported()


# ------------------------------------------------------------------ the parser, held to literals
# The binding's argument lists ARE the parser's output, so what can go wrong is the parser.  These are written by hand.
# <return>:<arguments> with i int, u unsigned, f float, d double, z size_t, p any pointer, v void, s const char*
SIGNATURES = {
    # the entry points the binding used to leave without argtypes, or with the default int for a void return
    "ofdis_last_error": "s:", "ofdis_version": "i:", "ofdis_build_id": "s:", "ofdis_device_count": "i:", "ofdis_set_device": "i:i",
    "ofdis_device_pci_bus_id": "i:ipi", "ofdis_flow_cache_clear": "v:", "ofdis_batch_destroy": "v:p", "ofdis_dev_free": "v:p",
    "ofdis_track_select_defaults": "v:p",
    # every size_t return
    "ofdis_encoding_bytes": "z:i", "ofdis_dense_tracks_work_bytes": "z:iiii", "ofdis_track_select_work_bytes": "z:i",
    "ofdis_codebook_train_work_bytes": "z:iiii", "ofdis_global_motion_work_bytes": "z:iii", "ofdis_batch_input_elems": "z:pi",
    "ofdis_batch_initflow_elems": "z:p", "ofdis_batch_device_bytes": "z:p",
    # pointer returns: only const char* is a string
    "ofdis_dev_alloc": "p:z", "ofdis_stream_create": "p:", "ofdis_batch_flow": "p:p", "ofdis_batch_input": "p:pii",
    # unsigned, double and size_t among the arguments
    "ofdis_batch_create_ex": "i:ppiu", "ofdis_camera_path": "i:pipidpp", "ofdis_batch_stabilize": "i:ppiiiififfpidipppiip",
    "ofdis_encode": "i:ppzpp", "ofdis_batch_build_pyramids_u8_seq": "i:ppzziip", "ofdis_global_motion": "i:ppiiiiifpppzp",
    "ofdis_dense_tracks": "i:pppiiiiiiiiffipppppzp", "ofdis_codebook_update": "i:ppppiiiiipppzp",
    "ofdis_codebook_train": "i:pppiiiiiipppppzp", "ofdis_batch_kernel_time": "i:pipp",
}
NARGS = {"ofdis_descriptor_normalize": 7, "ofdis_codebook_assign": 10, "ofdis_bof_histogram": 8, "ofdis_track_bof": 12,
         "ofdis_codebook_train_work_bytes": 4, "ofdis_codebook_seed": 10, "ofdis_codebook_update": 14, "ofdis_codebook_train": 16,
         "ofdis_track_descriptors": 19, "ofdis_track_select": 23}
ARGUMENTS = {("ofdis_codebook_update", 12): C.c_size_t, ("ofdis_codebook_train", 14): C.c_size_t,
             ("ofdis_camera_path", 4): C.c_double, ("ofdis_batch_create_ex", 3): C.c_uint}
RETURN_TEXT = {"ofdis_last_error", "ofdis_build_id"}
RETURN_NOTHING = {"ofdis_flow_cache_clear", "ofdis_batch_destroy", "ofdis_dev_free", "ofdis_host_free", "ofdis_stream_destroy",
                  "ofdis_event_destroy", "ofdis_track_select_defaults"}
RETURN_POINTERS = {"ofdis_dev_alloc", "ofdis_host_alloc", "ofdis_stream_create", "ofdis_event_create", "ofdis_batch_input",
                   "ofdis_batch_flow", "ofdis_batch_level_flow", "ofdis_batch_flow_reverse", "ofdis_batch_level_flow_reverse",
                   "ofdis_batch_flow_mirror", "ofdis_batch_level_flow_mirror"}
# declarations as they stand in the header, comments taken out and white space folded
DECLARED_TEXT = ["double* models, long long* stats, void* work, size_t work_bytes",
                 "const double* weights , int radius, double zoom",   # (the weights are a host array, said in a comment)
                 "uint8_t* out, uint8_t* inside , double* warps , int width_org, int height_org, void* stream"]
_CTYPE = {"i": C.c_int, "u": C.c_uint, "f": C.c_float, "d": C.c_double, "z": C.c_size_t, "p": C.c_void_p, "v": None,
          "s": C.c_char_p}


@pytest.mark.parametrize("name", SIGNATURES)
def test_the_parser_gives_the_signatures_written_here(name):
    ret, args = SIGNATURES[name].split(":")
    assert PROTOTYPES[name] == (_CTYPE[ret], [_CTYPE[a] for a in args])


def test_the_parser_gives_the_counts_and_types_written_here():
    for name, n in NARGS.items():
        assert len(PROTOTYPES[name][1]) == n, name
    for (name, at), ctype in ARGUMENTS.items():
        assert PROTOTYPES[name][1][at] is ctype, (name, at)
    for name, (restype, _) in PROTOTYPES.items():   # every return type: the few that are not int are named here
        want = (C.c_size_t if name.endswith(("_bytes", "_elems")) else C.c_char_p if name in RETURN_TEXT else
                None if name in RETURN_NOTHING else C.c_void_p if name in RETURN_POINTERS else C.c_int)
        assert restype is want, name
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", abi.header(), flags=re.S))
    for text in DECLARED_TEXT:
        assert text in flat, text


def test_the_parser_on_text_of_its_own():
    text = ("/* int ofdis_ghost(int a); */\nint ofdis_a(void);\nvoid ofdis_b();\n"
            "const char* ofdis_c(const float* const* x /* or NULL */,\n                    size_t n, unsigned flags);\n"
            "const float *ofdis_d(double z, float f);\n")
    assert prototypes(text) == {"ofdis_a": (C.c_int, []), "ofdis_b": (None, []),
                                "ofdis_c": (C.c_char_p, [C.c_void_p, C.c_size_t, C.c_uint]),
                                "ofdis_d": (C.c_void_p, [C.c_double, C.c_float])}
    assert list(prototypes(text)) == ["ofdis_a", "ofdis_b", "ofdis_c", "ofdis_d"]   # header order
    with pytest.raises(ValueError, match="ofdis_bad.*short x"):
        prototypes("int ofdis_bad(int a, short x);")
    with pytest.raises(ValueError, match="ofdis_worse.*short"):
        prototypes("short ofdis_worse(void);")
    with pytest.raises(ValueError, match="ofdis_unnamed"):
        prototypes("int ofdis_unnamed(int);")


def test_a_missing_header_fails_loudly(monkeypatch):
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr("of_dis_amd.abi.HEADER_PATH", "/nonexistent/ofdis.h")
    with pytest.raises(capi.OfdisError, match="ofdis.h"):
        capi.lib()


# ------------------------------------------------------------------ constants
CONSTANTS = {**abi.defines(), **abi.enumerators()}
MODELS = (gmotion, temporal, tracking, stabilize, encoding)   # the numpy model modules mirror the constants they use
# the values earlier tests pinned, and the status codes
PINNED = {"OFDIS_VERSION": 3, "OFDIS_OK": 0, "OFDIS_ERR_INVALID": -1, "OFDIS_ERR_UNSUPPORTED": -2, "OFDIS_ERR_DEVICE": -3,
          "OFDIS_ERR_NOMEM": -4, "OFDIS_BATCH_STEREO_LR": 2, "OFDIS_BATCH_SEQUENCE": 16, "OFDIS_FILL_NONE": 0,
          "OFDIS_FILL_INVALIDATE": 1, "OFDIS_FILL_BACKGROUND": 2, "OFDIS_DT_MAX_TRACKS": 1 << 24, "OFDIS_DT_MAX_STRIDE": 64,
          "OFDIS_DT_MAX_WINDOW": 7, "OFDIS_TS_KEPT": 0, "OFDIS_TS_SHORT": 1, "OFDIS_TS_INVALID": 2, "OFDIS_TS_STATIC": 3,
          "OFDIS_TS_ERRATIC": 4, "OFDIS_TS_JUMP": 5, "OFDIS_TS_CAMERA": 6, "OFDIS_TS_ALL_TESTS": 0x3F, "OFDIS_DESC_MAX_PATCH": 64,
          "OFDIS_BOF_SCALE": 510, "OFDIS_BOF_MAX_WORDS": 16384, "OFDIS_KMEANS_MAX_ITERS": 1000, "OFDIS_TRAJ_MAX_RADIUS": 8,
          "OFDIS_GM_MAX_SIDE": 8192, "OFDIS_GM_MAX_FLOW": 4096.0, "OFDIS_GM_MAX_ROUNDS": 8, "OFDIS_GM_TRANSLATION_ONLY": 0,
          "OFDIS_GM_AFFINE": 1, "OFDIS_GM_OK_AFFINE": 0, "OFDIS_GM_TRANSLATION": 1, "OFDIS_GM_EMPTY": 2, "OFDIS_GM_INLIER": 0,
          "OFDIS_GM_OUTLIER": 1, "OFDIS_GM_INVALID": 2, "OFDIS_STAB_MAX_RADIUS": 64, "OFDIS_STAB_MIN_DET": 0.25,
          "OFDIS_STAB_MAX_DET": 4.0, "OFDIS_STAB_MAX_ZOOM": 16.0, "OFDIS_BORDER_CONSTANT": 0, "OFDIS_BORDER_REPLICATE": 1}


def _twin(name):
    """the binding's name of a header constant: without the prefix (OFDIS_VERSION keeps it)"""
    return name if name == "OFDIS_VERSION" else name[len("OFDIS_"):]


@pytest.mark.parametrize("name", CONSTANTS)
def test_every_header_constant_has_an_equal_twin(name):
    value = CONSTANTS[name]
    assert hasattr(capi, _twin(name)), f"capi.{_twin(name)} is missing (include/ofdis.h: {name} = {value})"
    assert getattr(capi, _twin(name)) == value and type(getattr(capi, _twin(name))) is type(value), name
    for model in MODELS:
        if hasattr(model, _twin(name)):
            assert getattr(model, _twin(name)) == value, (model.__name__, name)
    if name in PINNED:
        assert value == PINNED[name], name


def test_the_constants_are_all_found():
    assert set(PINNED) <= set(CONSTANTS), set(PINNED) - set(CONSTANTS)
    assert len(abi.defines()) == 25 and len(abi.enumerators()) == 41 and not set(abi.defines()) & set(abi.enumerators())
    assert [abi.define(n) for n in ("OFDIS_BATCH_REVERSE", "OFDIS_FB_ALPHA", "OFDIS_TS_ALL_TESTS", "OFDIS_TRACK_MAX_POINTS")] \
        == [1, 0.01, 63, 1 << 24]   # the u, f, hex and shift spellings
    assert abi.enumerator("OFDIS_ERR_NOMEM") == -4 and abi.enumerator("OFDIS_K_COUNT") == 8
    # the selection codes: seven, 0 .. 6
    assert sorted(v for n, v in CONSTANTS.items() if n.startswith("OFDIS_TS_") and n != "OFDIS_TS_ALL_TESTS") == list(range(7))


def test_library_exports_every_declared_symbol():
    L = capi.lib()
    for name in _declared_functions():
        assert hasattr(L, name), f"{name} declared in include/ofdis.h but not exported"
    hdr = open(os.path.join(ROOT, "include", "ofdis.h")).read()
    assert L.ofdis_version() == capi.OFDIS_VERSION == int(re.search(r"#define OFDIS_VERSION (\d+)", hdr).group(1))


def test_build_id_is_the_hash_of_the_sources():
    """ofdis_build_id(): the library says which kernel sources + compiler flags it was built from (of_dis_amd.build.source_id);
    profiles/traffic_*.json carries the id of the library its counters were collected on and bench.py attaches it only to that
    library.  Here: the built library's id is the id of the tree it sits in (i.e. the build is not stale), and an id changes
    when a flag does."""
    from of_dis_amd import build
    assert capi.build_id() == build.source_id(), "libofdis_hip.so is stale: python -m of_dis_amd.build"
    assert build.source_id(extra_flags={"ofdis_dis.hip": ["-DX"]}) != build.source_id()
    import json
    for name in ("traffic_fused.json", "traffic_exact.json"):
        path = os.path.join(ROOT, "profiles", name)
        if os.path.exists(path):
            tj = json.load(open(path))
            assert "bytes_per_step" in tj and isinstance(tj.get("build_id", ""), str)


def test_binding_refuses_a_library_of_another_abi_version(monkeypatch):
    """The struct layouts of the binding belong to one ABI version: a stale libofdis_hip.so must not be handed our structs."""
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "OFDIS_VERSION", capi.OFDIS_VERSION + 1)
    with pytest.raises(capi.OfdisError, match="ABI version"):
        capi.lib()


def test_library_exports_nothing_but_the_header():
    """The shipped library's dynamic symbol table is exactly include/ofdis.h: no test hooks, no kernel handles, no C++
    internals (of_dis_amd/build.py links with a version script generated from the header; the parity tests' helper
    kernels live in the separate libofdis_testhooks.so)."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert exported == _declared_functions(), sorted(set(exported) ^ set(_declared_functions()))


def test_tuning_struct_layout_matches_header():
    src = open(os.path.join(ROOT, "include", "ofdis.h")).read()
    body = re.search(r"typedef struct ofdis_tuning \{(.*?)\} ofdis_tuning;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [d.split()[-1] for d in body.split(";") if d.strip()]
    assert names == [n for n, _ in capi.OfdisTuning._fields_]
    t = capi.get_tuning()   # host only: read from the environment, no device work
    assert (t.gray8, t.fused_tv, t.rgb12_lpp, t.contract, t.fused_tp_pipe) == (1, 1, 0, 0, 1)


def test_tuning_environment_variables_match_header():
    """Every knob of ofdis_tuning names the environment variable that initialises it; the library must read exactly those
    (and only in its one-time initialisation: no getenv on a launch path)."""
    src = open(os.path.join(ROOT, "include", "ofdis.h")).read()
    body = re.search(r"typedef struct ofdis_tuning \{(.*?)\} ofdis_tuning;", src, re.S).group(1)
    documented = set(re.findall(r"OFDIS_[A-Z0-9_]+", body))
    csrc = os.path.join(ROOT, "of_dis_amd", "csrc")
    knobs_src = open(os.path.join(csrc, "ofdis_context.hip")).read()
    init = knobs_src[knobs_src.index("void tuning_init_locked()"):knobs_src.index("ofdis_tuning tuning(unsigned* epoch)")]
    assert set(re.findall(r'"(OFDIS_[A-Z0-9_]+)"', init)) == documented
    for name in os.listdir(csrc):
        if name.endswith((".hip", ".h")):
            text = open(os.path.join(csrc, name)).read()
            if name == "ofdis_context.hip":
                text = text.replace(init, "")
            code = re.sub(r"//[^\n]*", "", text)  # (comments may mention it)
            # the one exception: the scratch-poisoning TEST HOOK, read where a context allocates its memory (never on a launch
            # path; the tests switch it on and off while the library is loaded)
            code = code.replace('getenv("OFDIS_POISON_SCRATCH")', "")
            assert "getenv(" not in code, f"{name} reads the environment outside the tuning initialisation"


def test_params_struct_layout_matches_header():
    src = open(os.path.join(ROOT, "include", "ofdis.h")).read()
    body = re.search(r"typedef struct ofdis_params \{(.*?)\} ofdis_params;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        fields += [(n.strip(), typ) for n in names.split(",")]
    assert [n for n, _ in fields] == [n for n, _ in OfdisParams._fields_]
    for (n, typ), (_, ct) in zip(fields, OfdisParams._fields_):
        assert (typ == "float") == (ct is C.c_float), n
    assert C.sizeof(OfdisParams) == 4 * len(fields)


@pytest.mark.parametrize("op", [1, 2, 3, 4])
@pytest.mark.parametrize("width", [1024, 640, 1920, 320])
def test_oppoint_table_matches_c_abi(op, width):
    """ofdis_params_oppoint (C++) and params.oppoint (Python) both restate run_dense.cpp:225-265."""
    q = OfdisParams()
    capi.check(capi.lib().ofdis_params_oppoint(C.byref(q), op, width, 1))
    p = oppoint(op, width, 436, verbosity=2)
    for name in ("sc_f", "sc_l", "max_iter", "min_iter", "p_samp_s", "usetvref", "imgpadding", "costfct", "patnorm",
                 "usefbcon", "tv_innerit", "tv_solverit", "verbosity", "noc"):
        assert getattr(p, name) == getattr(q, name), name
    for name in ("dp_thresh", "dr_thresh", "res_thresh", "patove", "tv_alpha", "tv_gamma", "tv_delta", "tv_sor"):
        assert np.float32(getattr(p, name)) == np.float32(getattr(q, name)), name


def test_readme_operating_point_2():
    """README.md:51-67: op-point 2 == `5 3 12 12 0.05 0.95 0 8 0.40 0 1 0 1 10 10 5 1 3 1.6 2` at width 1024."""
    p = oppoint(2, 1024, 436, verbosity=2)
    assert (p.sc_f, p.sc_l, p.max_iter, p.min_iter) == (5, 3, 12, 12)
    assert (p.p_samp_s, p.usefbcon, p.patnorm, p.costfct, p.usetvref) == (8, 0, 1, 0, 1)
    assert (p.tv_innerit, p.tv_solverit, p.verbosity) == (1, 3, 2)
    assert np.float32(p.patove) == np.float32(0.4) and np.float32(p.tv_sor) == np.float32(1.6)
    assert (p.width, p.height) == (1024, 448)
    assert auto_first_scale(1024, 5, 8) == 5


def test_geometry_matches_survey_table():
    """level sizes and patch counts of the BASELINE configs."""
    p = oppoint(2, 1024, 436)
    assert [p.level_size(l) for l in (5, 4, 3)] == [(32, 14), (64, 28), (128, 56)]
    assert p.steps == 4
    assert [p.grid(l)[0] * p.grid(l)[1] for l in (5, 4, 3)] == [32, 112, 448]
    p = oppoint(2, 640, 480)
    assert (p.width, p.height) == (640, 480)
    assert [p.level_size(l) for l in (5, 4, 3)] == [(20, 15), (40, 30), (80, 60)]
    assert [p.grid(l)[0] * p.grid(l)[1] for l in (5, 4, 3)] == [20, 80, 300]
    assert oppoint(1, 1024, 436).steps == 5          # 8*(1-0.3f) = 5.6 -> 5
    assert oppoint(4, 1920, 1080, noc=3).steps == 3  # 12*(1-0.75f) = 3
    assert padded_size(1920, 1080, 6) == (1920, 1088)


def test_status_codes_without_a_gpu():
    """Argument validation happens before any device work, so it is testable here."""
    L = capi.lib()
    h = C.c_void_p()
    p = oppoint(2, 1024, 436)
    for bad, code in ((p.copy(width=1000), -1), (p.copy(imgpadding=4), -1),
                      (p.copy(noc=2), -1), (p.copy(sc_l=6), -1), (p.copy(costfct=10), -2)):
        rc = L.ofdis_batch_create(C.byref(h), C.byref(bad), 4)
        assert rc == code, (bad.as_dict(), rc, L.ofdis_last_error())
        assert L.ofdis_last_error()
    assert L.ofdis_batch_create(C.byref(h), C.byref(p), 0) == -1


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", "/nonexistent/libofdis_hip.so")
    with pytest.raises(capi.OfdisError):
        capi.lib()


def test_outlier_threshold_is_the_exact_square_root_boundary():
    """The patch kernels test ||d||^2 > X instead of sqrt(||d||^2) > t (patch.cpp:199): X must be the largest float
    whose correctly rounded square root is <= t, for every patch size's t = P/2 and for awkward values."""
    import numpy as np
    from common import testhooks
    L = testhooks()
    f32 = np.float32
    for t in [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 13.0, 0.1, 0.7, 1e-3, 123.456, 3.4e18, 1e-19, 0.0]:
        t = f32(t)
        X = f32(L.ofdis_test_outlier_sq(t))
        up = np.nextafter(X, f32(np.inf))
        assert np.sqrt(X) <= t, (t, X)
        assert np.sqrt(up) > t, (t, X, up)
    assert np.isnan(L.ofdis_test_outlier_sq(float("nan")))
