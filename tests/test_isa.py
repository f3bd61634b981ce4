"""Static checks on the built gfx950 code object (no GPU needed): no kernel spills registers or uses scratch memory, and the
hot kernels keep the register budgets their occupancy figures in DESIGN.md rest on."""
import os
import re
import subprocess
import tempfile

import pytest

from of_dis_amd import build as B

def _llvm_bin():
    """The ROCm LLVM tools next to the hipcc that builds the library ($ROCM_PATH, hipcc's own tree, /opt/rocm)."""
    import shutil
    cands = []
    if os.environ.get("ROCM_PATH"):
        cands.append(os.path.join(os.environ["ROCM_PATH"], "lib", "llvm", "bin"))
    try:
        hipcc = os.path.realpath(B._hipcc())
        cands.append(os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin"))
    except RuntimeError:
        pass
    cands.append("/opt/rocm/lib/llvm/bin")
    for c in cands:
        if os.path.exists(os.path.join(c, "llvm-readelf")) and os.path.exists(os.path.join(c, "clang-offload-bundler")):
            return c
    return None


def _kernel_notes():
    """{mangled kernel name: metadata map} of every gfx950 kernel in the built library.  The metadata is the YAML document
    of the code objects' NT_AMDGPU_METADATA notes, parsed as YAML (no assumptions about key order); every kernel descriptor
    symbol (*.kd) of the code objects must have an entry."""
    import yaml
    llvm = _llvm_bin()
    so = B.lib_path()
    if not os.path.exists(so):
        B.build()
    tmp = tempfile.mkdtemp()
    fb = os.path.join(tmp, "fatbin")
    subprocess.check_call([llvm + "/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fb])
    blob = open(fb, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)]   # one bundle per translation unit
    kernels, descriptors = {}, set()
    for i, st in enumerate(starts):
        part, co = os.path.join(tmp, "bundle%d" % i), os.path.join(tmp, "gfx950_%d.co" % i)
        with open(part, "wb") as f:
            f.write(blob[st:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        subprocess.check_call([llvm + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + part,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        notes = subprocess.run([llvm + "/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
        for doc in re.findall(r"^\s*---\n(.*?)^\s*\.\.\.\s*$", notes, flags=re.S | re.M):
            meta = yaml.safe_load(doc)
            for k in (meta or {}).get("amdhsa.kernels", []):
                kernels[k[".name"]] = {key.lstrip("."): val for key, val in k.items()}
        syms = subprocess.run([llvm + "/llvm-readelf", "--symbols", "--wide", co], capture_output=True, text=True, check=True).stdout
        descriptors |= {m.group(1) for m in re.finditer(r"\s(\S+)\.kd\s*$", syms, flags=re.M)}
    missing = descriptors - set(kernels)
    assert not missing, f"kernel descriptors without metadata: {sorted(missing)[:5]}"
    return kernels


@pytest.fixture(scope="module")
def kernels():
    if _llvm_bin() is None:
        pytest.skip("ROCm LLVM tools not found")
    k = _kernel_notes()
    assert len(k) > 40, len(k)
    return k


# the 1024-thread lock-step SOR, sor_kernel<3, 3, 1024> (levels of 641 ... 1024 rows: 16 wavefronts of one workgroup on a CU = 128
# VGPRs each) is the one kernel allowed to spill; every kernel of the benchmarked configurations must not.  The entry carries the
# length prefix of the mangled name, so that it does not match the stereo de_sor_kernel<3, 3, 1024>, which must stay spill-free
# ... and the exact contract's 16-lanes-per-patch RGB kernel: squeezed into 168 registers for three wavefronts per SIMD it
# spills 9 of them (40 bytes of scratch) and is still 22 % faster than at 177 registers and two wavefronts (configs[3], exact
# contract: patch search 119 against 141 ms per 96 pairs; the one-patch-per-wavefront kernel: 153)
# ... and the fused contract's: with the template's y gradient in LDS it fits 168 registers for three wavefronts per SIMD
# except for 2 registers spilled OUTSIDE the iteration loop (template set-up and the final stores; no scratch access between
# the loop's first and last instruction): configs[3] at 96 pairs 82.4 -> 76.9 ms on one box
SPILL_OK = ("10sor_kernelILi3ELi3ELi1024EE", "patch_optimize_rgb12x_kernel", "patch_optimize_rgb12_kernel")


def test_no_kernel_spills_or_uses_scratch(kernels):
    sor = sorted(n for n in kernels if SPILL_OK[0] in n)  # the flow <3, 3, 1024> build, once per arithmetic contract, nothing else
    assert len(sor) == 2 and "5exact" in sor[0] and "5fused" in sor[1], sor
    for name, m in kernels.items():
        if any(s in name for s in SPILL_OK):
            continue
        assert int(m["vgpr_spill_count"]) == 0, (name, m)
        assert int(m["sgpr_spill_count"]) == 0, (name, m)
        assert int(m["private_segment_fixed_size"]) == 0, (name, m)


@pytest.mark.parametrize("pattern,max_vgprs,what", [
    # (three wavefronts per SIMD -- 168 registers, forced with a launch bound -- measured 5 % slower than the 181 the compiler
    # takes by itself: profiles/README.md round 3)
    ("tv_fused_kernelILi3ELb1ELi0ELi1EE", 192, "tv_fused_kernel<3, true, 0>, throughput mapping: two wavefronts per SIMD"),
    ("tv_fused_kernelILi3ELb1ELi0ELi3EE", 256, "tv_fused_kernel<3, true, 0, 3>, RGB levels on the throughput mapping (derivative ring of two rows): two wavefronts per SIMD"),
    ("tv_fused_kernelILi3ELb1ELi1ELi3EE", 256, "tv_fused_kernel<3, true, 1, 3>, RGB levels on the iteration-pipelined mapping: two wavefronts per SIMD"),
    ("tv_fused_kernelILi3ELb1ELi2ELi1EE", 168, "tv_fused_kernel<3, true, 2>, split mapping: 12 wavefronts of a workgroup on one CU"),
    ("tv_fused_xcu_kernelILi3ELb1EE", 128, "tv_fused_xcu_kernel<3, true>, cross-CU mapping: one wavefront per SIMD, four workgroups per CU at most"),
    ("patch_optimize_gray8_kernelILi0ELb0EE", 128, "gray 8x8 patch kernel: four wavefronts per SIMD"),
    ("patch_optimize_kernelILi7ELi64ELi432ELi1EE", 84, "RGB 12x12 patch kernel, L1 cost: six wavefronts per SIMD"),
    ("patch_optimize_rgb12x_kernelILi1ELi3ELb0ELi3EE", 168, "RGB 12x12 patch kernel of the exact contract (blocks for the taps, chains for the sums): three wavefronts per SIMD"),
    ("patch_optimize_rgb12_kernelILi1ELi3ELb0ELi3EE", 168, "RGB 12x12 patch kernel of the fused contract (3x3 pixel block per lane, Ty in LDS): three wavefronts per SIMD"),
    ("tv_fused_kernelILi3ELb1ELi1ELi1EE", 168, "tv_fused_kernel<3, true, 1>, iteration-pipelined mapping: three wavefronts per SIMD (three workgroups of four iterations per CU)"),
    ("tv_fused_tall_kernelILi3ELb1ELb0ELi1EE", 216, "tv_fused_tall_kernel<3, true, false> (two to four wavefronts per strip, 65-256 rows): two wavefronts per SIMD"),
    ("tv_fused_tall_kernelILi3ELb1ELb1ELi1EE", 216, "tv_fused_tall_kernel<3, true, true> (heads + shared tail): two wavefronts per SIMD"),
    ("tv_fused_tall_kernelILi3ELb1ELb0ELi3EE", 256, "tv_fused_tall_kernel<3, true, false, 3>, RGB: two wavefronts per SIMD"),
    ("tv_fused_tall_kernelILi3ELb1ELb1ELi3EE", 256, "tv_fused_tall_kernel<3, true, true, 3>, RGB, heads + shared tail (eight wavefronts per workgroup: 256 registers at most)"),
    ("densify_kernelILb1ELi0EE", 64, "densify_kernel<true, 0>: eight wavefronts per SIMD"),
    ("densify_quad_kernel", 64, "densify_quad_kernel: eight wavefronts per SIMD"),
    ("tv_prep_kernelILi2ELb0EE", 84, "tv_prep_kernel<2, false> (two wavefronts per 128-column row): six wavefronts per SIMD by registers"),
    ("tv_prep_kernelILi1ELb0EE", 84, "tv_prep_kernel<1, false>: six wavefronts per SIMD by registers"),
    ("tv_prep_kernelILi2ELb1EE", 96, "tv_prep_kernel<2, true> (densification inside: twelve pending registers instead of two): five wavefronts per SIMD by registers"),
    ("tv_prep_kernelILi1ELb1EE", 96, "tv_prep_kernel<1, true>: five wavefronts per SIMD by registers"),
])
def test_register_budgets(kernels, pattern, max_vgprs, what):
    hits = [(n, m) for n, m in kernels.items() if pattern in n]
    assert hits, pattern
    for n, m in hits:
        assert int(m["vgpr_count"]) <= max_vgprs, (what, n, m["vgpr_count"])


def test_rgb12_fused_kernel_spills_only_outside_its_iteration_loop():
    """The fused contract's RGB 12x12 patch kernel is allowed two spilled registers (SPILL_OK above) because no scratch
    access lies inside its Gauss-Newton loop: checked on the disassembly (largest backward-branch loop of the kernel)."""
    llvm = _llvm_bin()
    if llvm is None:
        pytest.skip("ROCm LLVM tools not found")
    obj = os.path.join(os.path.dirname(B.lib_path()), "ofdis_dis.fused.o")
    if not os.path.exists(obj):
        B.build()
    tmp = tempfile.mkdtemp()
    fb, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.co")
    subprocess.check_call([llvm + "/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fb])
    subprocess.check_call([llvm + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fb,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    text = subprocess.run([llvm + "/llvm-objdump", "-d", "--demangle", co], capture_output=True, text=True, check=True).stdout
    checked = 0
    for m in re.finditer(r"^[0-9a-f]+ <(void ofdis::fused::patch_optimize_rgb12_kernel<\d, 3, \w+, 3>\(ofdis::DisArgs\))>:\n(.*?)(?=^[0-9a-f]+ <|\Z)",
                         text, flags=re.S | re.M):
        lines = [l for l in m.group(2).splitlines() if re.search(r"//\s*[0-9A-Fa-f]+:", l)]
        addr = [int(re.search(r"//\s*([0-9A-Fa-f]+):", l).group(1), 16) for l in lines]
        loops = []
        for i, l in enumerate(lines):
            b = re.match(r"\s+(s_cbranch_\w+|s_branch)\s+(\d+)", l)
            if b and int(b.group(2)) >= 32768:  # backward branch: target = next instruction + signed 16-bit word offset
                tgt = addr[i] + 4 + (int(b.group(2)) - 65536) * 4
                loops.append((i - addr.index(tgt), addr.index(tgt), i))
        assert loops, m.group(1)
        _, lo, hi = max(loops)
        assert hi - lo > 300, (m.group(1), lo, hi)  # the iteration loop, not a short wait loop
        inside = [l for l in lines[lo:hi + 1] if "scratch_" in l]
        assert not inside, (m.group(1), inside[:3])
        checked += 1
    assert checked == 4, checked  # COST = 0 (L2) and 1 (L1), flow and stereo


@pytest.mark.parametrize("pattern,blocks_per_cu,what", [
    ("tv_fused_kernelILi3ELb1ELi1ELi1EE", 3, "iteration-pipelined fused TV: three workgroups of four wavefronts per compute unit"),
    ("patch_optimize_rgb12_kernelILi1ELi3ELb0ELi3EE", 3, "fused contract's RGB 12x12 patch kernel: three blocks of four wavefronts per compute unit"),
    ("patch_optimize_rgb12x_kernelILi1ELi3ELb0ELi3EE", 3, "exact contract's RGB 12x12 patch kernel: three blocks of four wavefronts per compute unit"),
])
def test_lds_budgets(kernels, pattern, blocks_per_cu, what):
    """The occupancy these kernels were brought to by moving registers into LDS must not be taken away by the LDS itself
    (160 KB per compute unit on gfx950)."""
    names = [n for n in kernels if pattern in n]
    assert names, pattern
    for n in names:
        lds = int(kernels[n]["group_segment_fixed_size"])
        assert lds * blocks_per_cu <= 160 * 1024, (what, n, lds)


def test_committed_isa_counts_match_the_build():
    """profiles/isa_counts.json (bench.py prices the RGB patch search of BASELINE configs[3] against the VALU issue peak with
    these loop instruction counts) must be what tools/isa_count.py finds in the library that ships."""
    import json
    import sys
    if _llvm_bin() is None:
        pytest.skip("ROCm LLVM tools not found")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import isa_count
    if not os.path.exists(B.lib_path()):
        B.build()
    now = isa_count.profile_counts(os.path.dirname(B.lib_path()))
    committed = json.load(open(os.path.join(root, "profiles", "isa_counts.json")))
    assert set(now) == set(isa_count.PROFILE_KERNELS), sorted(now)
    for key, c in now.items():
        assert committed[key] == c, (key, committed[key], c, "refresh with: python tools/isa_count.py --write-profile")
