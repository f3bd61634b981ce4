"""Build the product: libofdis_hip.so (HIP kernels + C ABI, gfx950) and the run_OF_* executables.

    python -m of_dis_amd.build          # incremental
    python -m of_dis_amd.build --force

Everything is compiled in-tree (of_dis_amd/lib/) so that the built .so travels with the repo
snapshot to the GPU box.  hipcc cross-compiles gfx950 without a GPU.
"""
import os
import shutil
import subprocess
import sys

from .abi import prototypes

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
ROOT = os.path.dirname(HERE)

# Kernel files: compiled once per ARITHMETIC CONTRACT (csrc/ofdis_dev.h) from the same source, into ofdis::exact and
# ofdis::fused; the pyramid (exact by construction for 8-bit input), the full-resolution finish and frame interpolation (exact
# only: a fixed fp32 operation order, include/ofdis.h), the stereo left-right step, the point and dense trajectories, their selection and their
# descriptors, their bag-of-features encoding and the k-means training of its codebook (integers throughout), the temporal filters, the global motion models, the segments of label maps, their tracks and the stabiliser (exact only, likewise) and the C ABI are compiled once:
# the context (ofdis_context.hip), its launch schedule (ofdis_schedule.hip), what is made from its flows (ofdis_products.hip) and
# the rest (ofdis_capi.hip).
KERNEL_SOURCES = ["ofdis_dis.hip", "ofdis_tv.hip", "ofdis_prep.hip", "ofdis_sor.hip", "ofdis_fused.hip", "ofdis_fused_xcu.hip",
                  "ofdis_fused_tall.hip", "ofdis_de.hip"]
COMMON_SOURCES = ["ofdis_pyr.hip", "ofdis_upsample.hip", "ofdis_interp.hip", "ofdis_stereo_lr.hip", "ofdis_track.hip", "ofdis_dense_tracks.hip", "ofdis_track_select.hip", "ofdis_descriptors.hip", "ofdis_bof.hip", "ofdis_kmeans.hip", "ofdis_tfilter.hip", "ofdis_trajfilter.hip", "ofdis_gmotion.hip",
                  "ofdis_segments.hip", "ofdis_segment_tracks.hip", "ofdis_stabilize.hip", "ofdis_context.hip", "ofdis_schedule.hip", "ofdis_products.hip", "ofdis_capi.hip"]
HIP_SOURCES = KERNEL_SOURCES + COMMON_SOURCES
# -fvisibility=hidden: the shared library exports the C ABI of include/ofdis.h (marked in ofdis_context.h) and nothing else.
BASEFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
             "-Wall", "-Wno-unused-function", "-Wno-bitwise-instead-of-logical"]
# exact: -ffp-contract=off, every fp32 operation separately rounded, like the reference's SSE path (bit-identical results).
# fused: the tolerance contract (EPE < 1e-3 px): a * b + c contracts into one v_fma_f32, also across statements.
CONTRACT_FLAGS = {"exact": ["-DOFDIS_CONTRACT=0", "-ffp-contract=off"],
                  "fused": ["-DOFDIS_CONTRACT=1", "-ffp-contract=fast"]}
HIPFLAGS = BASEFLAGS + CONTRACT_FLAGS["exact"]


# No SLP vectorisation: gfx950's SIMDs are 32 lanes wide, so a packed v_pk_*_f32 occupies the issue port about as
# long as the two scalar ops it replaces (tools/probes/valu_probe.hip: 4.2 vs 2 x 2.5 cycles per wave64) and the
# moves that assemble register pairs are pure overhead; in ofdis_dis.hip it also splits the DPP reduction chains.
_NO_SLP = ["-fno-slp-vectorize"]
PER_FILE_FLAGS = {"ofdis_dis.hip": _NO_SLP, "ofdis_tv.hip": _NO_SLP, "ofdis_prep.hip": _NO_SLP, "ofdis_fused.hip": _NO_SLP,
                  "ofdis_fused_xcu.hip": _NO_SLP, "ofdis_fused_tall.hip": _NO_SLP,
                  "ofdis_sor.hip": _NO_SLP}


# The product's units the TEST library links as well (testhooks_path), compiled a second time with TESTHOOK_FLAGS.
TESTHOOK_UNITS = ["ofdis_interp.hip", "ofdis_tfilter.hip", "ofdis_trajfilter.hip", "ofdis_gmotion.hip", "ofdis_stabilize.hip",
                  "ofdis_upsample.hip", "ofdis_stereo_lr.hip", "ofdis_pyr.hip", "ofdis_bof.hip", "ofdis_kmeans.hip",
                  "ofdis_track.hip", "ofdis_dense_tracks.hip", "ofdis_segments.hip"]
TESTHOOK_FLAGS = ["-DOFDIS_TEST_LAUNCH_LIMITS"]


def _hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def abi_symbols():
    """Every function include/ofdis.h declares: the export list of the shared library."""
    return sorted(prototypes())


def source_id(csrc=None, extra_flags=None):
    """Identity of what the kernels of a build are made of: a hash over every kernel / header source under csrc/ (not the
    host/ mains), include/ofdis.h and the compiler flags above.  It is compiled into the library (ofdis_build_id()) and
    stamped into profiles/traffic_*.json when the PMC counters are collected: bench.py attaches counter-derived figures only
    to a library with the SAME id -- a kernel change without a PMC re-run cannot keep a stale roofline fraction."""
    import hashlib
    csrc = csrc or CSRC
    h = hashlib.sha256()
    names = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".inc")))
    for name in names:
        h.update(name.encode() + b"\0")
        h.update(open(os.path.join(csrc, name), "rb").read())
    h.update(open(os.path.join(ROOT, "include", "ofdis.h"), "rb").read())
    h.update(repr((BASEFLAGS, sorted(CONTRACT_FLAGS.items()), sorted(PER_FILE_FLAGS.items()),
                   sorted((extra_flags or {}).items()))).encode())
    return h.hexdigest()[:16]


def _build_id_header(csrc, outdir, extra_flags=None):
    """outdir/ofdis_build_id.h (included by ofdis_capi.hip), rewritten only when the id changes."""
    path = os.path.join(outdir, "ofdis_build_id.h")
    text = f'#define OFDIS_BUILD_ID "{source_id(csrc, extra_flags)}"\n'
    if not os.path.exists(path) or open(path).read() != text:
        open(path, "w").write(text)
    return path


def _version_script():
    """Linker version script exporting include/ofdis.h and nothing else (kernel handles, inline members of the context
    struct and the runtime's registration symbols stay local)."""
    path = os.path.join(LIBDIR, "ofdis.map")
    text = "{\n  global:\n" + "".join(f"    {n};\n" for n in abi_symbols()) + "  local: *;\n};\n"
    if not os.path.exists(path) or open(path).read() != text:
        open(path, "w").write(text)
    return path


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
    if verbose and (r.stdout or r.stderr):
        print(r.stdout + r.stderr)


def lib_path():
    return os.path.join(LIBDIR, "libofdis_hip.so")


def testhooks_path():
    """The TEST library: kernels that expose header-only helpers to the parity tests (tests/csrc/ofdis_testhooks.hip) and the
    product's post-processing launchers with lowered launch limits (tests/csrc/ofdis_launch_hooks*.hip, TESTHOOK_UNITS).
    Built next to the product, never linked into it."""
    return os.path.join(LIBDIR, "libofdis_testhooks.so")


IO_PROBE_SOURCES = [os.path.join(ROOT, "tests", "c", "image_io_probe.cpp"), os.path.join(CSRC, "host", "image_io.cpp")]


def io_probe_path():
    """The stand-alone program around host/image_io.cpp that tests/test_image_io.py feeds its files to."""
    return os.path.join(LIBDIR, "image_io_probe")


def io_probe_command(exe, extra_flags=()):
    """The host compiler's command line for the probe (tools/host_sanitize.sh builds a second one with sanitizer flags)."""
    return ["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra"] + list(extra_flags) + ["-I", os.path.join(CSRC, "host")] + \
        IO_PROBE_SOURCES + ["-o", exe, "-lz"]


# The host executables: main file -> (program, OFDIS_NOC, OFDIS_MODE).  Every program links its main and HOST_COMMON, nothing
# else: a new .cpp under host/ belongs to one of the two lists, by name.
HOST_DIR = os.path.join(CSRC, "host")
HOST_COMMON = ["image_io.cpp"]
HOST_MAINS = {"run_dense_main.cpp": (("run_OF_INT", 1, 1), ("run_OF_RGB", 3, 1), ("run_DE_INT", 1, 2), ("run_DE_RGB", 3, 2)),
              "run_seq_main.cpp": (("run_OF_INT_seq", 1, 1), ("run_OF_RGB_seq", 3, 1), ("run_DE_INT_seq", 1, 2),
                                   ("run_DE_RGB_seq", 3, 2))}


def host_sources(main_name):
    return [os.path.join(HOST_DIR, f) for f in [main_name] + HOST_COMMON]


# The sequence driver linked against tests/c/ofdis_abi_stub.c instead of the library: no HIP runtime, runs without a GPU
# (tests/test_seq_driver_stub.py).  program -> (OFDIS_NOC, OFDIS_MODE)
SEQ_STUB_SOURCE = os.path.join(ROOT, "tests", "c", "ofdis_abi_stub.c")
SEQ_STUB_PROGRAMS = {"run_OF_INT_seq_stub": (1, 1), "run_DE_RGB_seq_stub": (3, 2)}


def seq_stub_path(name):
    return os.path.join(LIBDIR, name)


def seq_stub_commands(exe, name, extra_flags=()):
    """The host compilers' command lines for a stub-linked driver: the stub as C, then the driver's own sources as C++ with it
    (tools/host_sanitize.sh builds further pairs with sanitizer flags)."""
    noc, mode = SEQ_STUB_PROGRAMS[name]
    flags = ["-O2", "-g", "-Wall", "-Wextra", "-pthread"] + list(extra_flags) + ["-I", os.path.join(ROOT, "include")]
    obj = exe + ".stub.o"
    return [["gcc", "-std=c11"] + flags + ["-c", SEQ_STUB_SOURCE, "-o", obj],
            ["g++", "-std=c++17"] + flags + [f"-DOFDIS_NOC={noc}", f"-DOFDIS_MODE={mode}"] + host_sources("run_seq_main.cpp")
            + [obj, "-o", exe, "-lm", "-lz"]]


def compile_units(csrc, outdir, force=False, verbose=False, extra_flags=None, only=None):
    """Compile every translation unit of the library (kernel files once per contract) from `csrc` into `outdir`; returns
    the object list.  extra_flags: {file name: [flags]} on top of PER_FILE_FLAGS (developer A/B builds, tools/ab_build.py).
    only: the file names to compile instead of all of them (the test library links a few of the product's units)."""
    hipcc = _hipcc()
    headers = [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith((".h", ".inc"))]
    headers.append(os.path.join(ROOT, "include", "ofdis.h"))
    headers.append(os.path.abspath(__file__))  # the flags live here
    build_id_h = _build_id_header(csrc, outdir, extra_flags)  # changes whenever any kernel source or flag does
    objs, jobs = [], []
    units = [(src, c) for c in ("exact", "fused") for src in KERNEL_SOURCES] + [(src, "exact") for src in COMMON_SOURCES]
    if only is not None:
        units = [(src, c) for src, c in units if src in only]
    for src, contract in units:
        sp = os.path.join(csrc, src)
        suffix = ".o" if contract == "exact" else "." + contract + ".o"
        obj = os.path.join(outdir, src.replace(".hip", suffix))
        deps = [sp] + headers + ([build_id_h] if src == "ofdis_capi.hip" else [])
        if force or _newer(obj, deps):
            flags = PER_FILE_FLAGS.get(src, []) + (extra_flags or {}).get(src, [])
            if src == "ofdis_capi.hip":
                flags = flags + ["-I", outdir]
            jobs.append([hipcc] + BASEFLAGS + CONTRACT_FLAGS[contract] + flags + ["-c", sp, "-o", obj])
        objs.append(obj)
    if jobs:  # the translation units are independent: compile them side by side
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as ex:
            list(ex.map(lambda cmd: _run(cmd, verbose), jobs))
    return objs, headers


def build(force=False, verbose=False):
    os.makedirs(LIBDIR, exist_ok=True)
    hipcc = _hipcc()
    objs, headers = compile_units(CSRC, LIBDIR, force, verbose)
    so = lib_path()
    vs = _version_script()
    if force or _newer(so, objs + [vs]):
        _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", f"-Wl,--version-script={vs}", "-o", so] + objs, verbose)
    # host executables: the reference's CLI contract (run_OF_INT / run_OF_RGB and the stereo-depth run_DE_INT / run_DE_RGB,
    # one pair per process: host/run_dense_main.cpp) and the sequence drivers (run_OF_*_seq / run_DE_*_seq: many pairs,
    # one host thread per GPU: host/run_seq_main.cpp), each with HOST_COMMON
    host_hdrs = [os.path.join(HOST_DIR, f) for f in os.listdir(HOST_DIR) if f.endswith(".h")] if os.path.isdir(HOST_DIR) else []
    for main_name, exes in HOST_MAINS.items():
        sources = host_sources(main_name)
        if not os.path.exists(sources[0]):
            continue
        for name, noc, mode in exes:
            exe = os.path.join(LIBDIR, name)
            if force or _newer(exe, sources + host_hdrs + headers + [so]):
                _run(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", f"-DOFDIS_NOC={noc}", f"-DOFDIS_MODE={mode}", "-I",
                      os.path.join(ROOT, "include")] + sources
                     + ["-o", exe, "-L", LIBDIR, "-lofdis_hip", "-lz", "-Wl,-rpath,$ORIGIN"], verbose)
    # test-only artefacts: a failure here must not take the product down with it (it is reported, the tests that need
    # them fail on their own)
    try:
        # the plain-C caller of the drop-in boundary (tests/c/dropin_test.c): compiled as C99 against include/ofdis.h
        c_test = os.path.join(ROOT, "tests", "c", "dropin_test.c")
        if os.path.exists(c_test):
            exe = os.path.join(LIBDIR, "dropin_test")
            if force or _newer(exe, [c_test, os.path.join(ROOT, "include", "ofdis.h"), so]):
                _run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-O2", "-D_POSIX_C_SOURCE=199309L", "-I",
                      os.path.join(ROOT, "include"), c_test, "-o", exe, "-L", LIBDIR, "-lofdis_hip", "-Wl,-rpath,$ORIGIN"],
                     verbose)
        # the host image readers and writers alone (tests/c/image_io_probe.cpp): image_io.cpp and zlib, no HIP runtime
        if os.path.exists(IO_PROBE_SOURCES[0]):
            exe = io_probe_path()
            if force or _newer(exe, IO_PROBE_SOURCES + [os.path.join(CSRC, "host", "image_io.h")]):
                _run(io_probe_command(exe), verbose)
        # the sequence driver on the host-only stand-in for the library (tests/c/ofdis_abi_stub.c)
        if os.path.exists(SEQ_STUB_SOURCE):
            for name in SEQ_STUB_PROGRAMS:
                exe = seq_stub_path(name)
                if force or _newer(exe, [SEQ_STUB_SOURCE, os.path.join(ROOT, "include", "ofdis.h")] + host_sources("run_seq_main.cpp")
                                   + host_hdrs):
                    for cmd in seq_stub_commands(exe, name):
                        _run(cmd, verbose)
        hooks = os.path.join(ROOT, "tests", "csrc", "ofdis_testhooks.hip")
        if os.path.exists(hooks):
            # the launch hooks (tests/csrc/ofdis_launch_hooks.hip) call the product's own launchers: TESTHOOK_UNITS compiled
            # with the product's flags plus the define that turns the two launch limits into variables of this library
            # (csrc/ofdis_kernels.h), into an object directory of their own
            tdir = os.path.join(LIBDIR, "testhooks")
            os.makedirs(tdir, exist_ok=True)
            tobjs, _ = compile_units(CSRC, tdir, force, verbose, {u: TESTHOOK_FLAGS for u in TESTHOOK_UNITS}, only=TESTHOOK_UNITS)
            hook_deps = headers + [os.path.join(ROOT, "tests", "csrc", "ofdis_test_hooks.h")]  # every hook's declaration
            # (ofdis_launch_hooks.hip and the files beside it that add one product's hooks: ofdis_launch_hooks_*.hip)
            lobjs = []
            for name in sorted(f for f in os.listdir(os.path.join(ROOT, "tests", "csrc"))
                               if f.startswith("ofdis_launch_hooks") and f.endswith(".hip")):
                launch_hooks = os.path.join(ROOT, "tests", "csrc", name)
                lobjs.append(os.path.join(tdir, name.replace(".hip", ".o")))
                if force or _newer(lobjs[-1], [launch_hooks] + hook_deps):
                    _run([hipcc] + HIPFLAGS + TESTHOOK_FLAGS + ["-c", launch_hooks, "-o", lobjs[-1]], verbose)
            hobj = os.path.join(tdir, "ofdis_testhooks.o")
            if force or _newer(hobj, [hooks] + hook_deps):
                _run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-c", hooks, "-o", hobj],
                     verbose)
            tso = testhooks_path()
            if force or _newer(tso, [hobj] + lobjs + tobjs):
                _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tso, hobj] + lobjs + tobjs, verbose)
    except RuntimeError as e:
        print("of_dis_amd.build: test artefacts not built:", str(e)[:2000], file=sys.stderr)
    return so


if __name__ == "__main__":
    p = build(force="--force" in sys.argv, verbose=True)
    print("built", p)
