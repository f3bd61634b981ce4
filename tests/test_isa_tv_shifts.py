"""Static check (no GPU needed) that the lane shifts of the fused TV kernel stay folded into the instructions that consume
them (ofdis_dev.h: mul_pairs_from_prev, fmac_pairs_from_next, vertical_terms): ofdis_fused.hip is cross-compiled to gfx950
assembly under both arithmetic contracts with the flags of of_dis_amd/build.py, and the step loops of the two headline
instantiations are counted.

The step loop is the largest backward-branch loop of a kernel; it is unrolled by U = 6 diagonal steps, so the figures per
step are the loop's divided by six.  A "bare move" is a v_mov_b32_dpp: a lane shift that is an instruction of its own.
Left as moves on purpose: the four flow neighbours of the smoothness term (each goes through a border select) and sv_t
(several consumers) -- five per step.
"""
import os
import re
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

from of_dis_amd import build as B

U = 6  # diagonal steps per pass of the unrolled step loop (tv_fused_kernel: constexpr int U)
MAX_BARE_MOVES_PER_STEP = 8
MODE1_MAX_VGPRS = 168  # three wavefronts per SIMD (the kernel's amdgpu_waves_per_eu)

# tv_fused_kernel<3, true, 0, 1> (levels 4, 5 of the headline) and <3, true, 1, 1> (level 3)
KERNELS = {0: "tv_fused_kernelILi3ELb1ELi0ELi1EE", 1: "tv_fused_kernelILi3ELb1ELi1ELi1EE"}

# (instructions, v_mov_b32_dpp) of one pass of the step loop at the parent commit a7745e3 ("Add dense trajectories:
# textured grid seeds, re-seeded every frame"), counted by this file's own functions on that commit's ofdis_fused.hip:
# per step 425.5 / 502.5 (exact) and 271.8 / 346.7 (fused) instructions, 18 (exact) and 20 (fused) bare moves
PARENT = {("exact", 0): (2553, 108), ("exact", 1): (3015, 108), ("fused", 0): (1631, 120), ("fused", 1): (2080, 120)}


def _assemble(contract, out):
    flags = B.BASEFLAGS + B.CONTRACT_FLAGS[contract] + B.PER_FILE_FLAGS.get("ofdis_fused.hip", [])
    cmd = [B._hipcc()] + flags + ["--cuda-device-only", "-S", os.path.join(B.CSRC, "ofdis_fused.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


@pytest.fixture(scope="module")
def asm():
    try:
        B._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    tmp = tempfile.mkdtemp()
    with ThreadPoolExecutor(max_workers=2) as ex:
        texts = list(ex.map(lambda c: _assemble(c, os.path.join(tmp, c + ".s")), ("exact", "fused")))
    return dict(zip(("exact", "fused"), texts))


def _kernel_body(text, pattern):
    """Lines of the one kernel whose mangled name contains `pattern`, from its label to the end of the function."""
    hits = [m for m in re.finditer(r"^(_Z\w+):", text, flags=re.M) if pattern in m.group(1)]
    assert len(hits) == 1, (pattern, [m.group(1) for m in hits])
    start = hits[0].end()
    return hits[0].group(1), text[start:text.index(".Lfunc_end", start)].splitlines()


def _step_loop(body):
    """[(opcode, operands)] of the largest backward-branch loop."""
    labels, ins = {}, []
    for line in body:
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        m = re.match(r"^\s+([a-z]\w+)\s*(.*?)(?:\s*;.*)?$", line)
        if m and not line.strip().startswith("."):
            ins.append((m.group(1), m.group(2)))
    best = None
    for i, (op, args) in enumerate(ins):
        if op.startswith("s_cbranch") or op == "s_branch":
            t = labels.get(args.strip())
            if t is not None and t <= i and (best is None or i - t > best[1] - best[0]):
                best = (t, i)
    assert best is not None
    return ins[best[0]:best[1] + 1]


def _metadata(text, name):
    import yaml
    doc = text[text.index(".amdgpu_metadata") + len(".amdgpu_metadata"):text.index(".end_amdgpu_metadata")]
    doc = doc[doc.index("---") + 3:doc.rindex("\n...")]  # the YAML document between its markers
    for k in yaml.safe_load(doc)["amdhsa.kernels"]:
        if k[".name"] == name:
            return k
    raise AssertionError(name)


@pytest.mark.parametrize("contract", ["exact", "fused"])
@pytest.mark.parametrize("mode", [0, 1])
def test_shifts_are_folded_into_their_consumers(asm, contract, mode):
    name, body = _kernel_body(asm[contract], KERNELS[mode])
    loop = _step_loop(body)
    total = len(loop)
    moves = sum(op == "v_mov_b32_dpp" for op, _ in loop)
    folded = sum(op.endswith("_dpp") and op != "v_mov_b32_dpp" for op, _ in loop)
    parent_total, parent_moves = PARENT[(contract, mode)]
    print(f"{contract} MODE {mode}: {total / U:.1f} instructions per step (parent {parent_total / U:.1f}), "
          f"{moves / U:.1f} bare v_mov_b32_dpp (parent {parent_moves / U:.1f}), {folded / U:.1f} shifts folded")
    assert total > 200 * U, (name, total)  # the step loop, not a short wait loop
    assert moves <= MAX_BARE_MOVES_PER_STEP * U, (name, moves / U)
    assert total < parent_total, (name, total / U, parent_total / U)


@pytest.mark.parametrize("contract", ["exact", "fused"])
@pytest.mark.parametrize("mode", [0, 1])
def test_no_scratch_and_register_budget(asm, contract, mode):
    name, _ = _kernel_body(asm[contract], KERNELS[mode])
    m = _metadata(asm[contract], name)
    assert int(m[".private_segment_fixed_size"]) == 0, (name, m)
    assert int(m[".vgpr_spill_count"]) == 0 and int(m[".sgpr_spill_count"]) == 0, (name, m)
    if mode == 1:
        assert int(m[".vgpr_count"]) <= MODE1_MAX_VGPRS, (name, m[".vgpr_count"])


@pytest.mark.parametrize("contract", ["exact", "fused"])
def test_no_valu_write_of_exec(asm, contract):
    """The folded shifts sit in asm statements that guard the VGPR hazard of a DPP read themselves (s_nop 1); the EXEC
    hazard (five wait states after a VALU write of EXEC) they leave to the fact that the compiler emits no v_cmpx here."""
    for line in asm[contract].splitlines():
        assert not re.match(r"^\s+v_cmpx", line), line
    # ... and every statement that folds a shift opens with its s_nop 1: a DPP arithmetic instruction is preceded, within
    # its statement (at most six instructions), by one
    for pattern in KERNELS.values():
        _, body = _kernel_body(asm[contract], pattern)
        ops = [m.group(1) + " " + m.group(2) for m in (re.match(r"^\s+([a-z]\w+)\s*(.*?)(?:\s*;.*)?$", l) for l in body)
               if m and not m.group(0).strip().startswith(".")]
        for i, op in enumerate(ops):
            if re.match(r"v_(fmac|sub|subrev|add)_f32_dpp ", op):  # (v_mul_f32_dpp: the compiler folds some of its own)
                assert any(o.startswith("s_nop 1") for o in ops[max(0, i - 6):i]), (pattern, ops[max(0, i - 7):i + 1])
