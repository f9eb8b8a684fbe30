"""The instance-group step kernel keeps its lane's item words of the flat LU program in registers for the whole launch (gridpf_sparse.hpp:
FlatWords), so the Newton loop of the 14-substation headline kernel performs NO load from global memory: the sweeps used to fetch the words
through L2 at the head of every sweep of every iteration of every step.

CPU check on the ISA of the grid-specialised headline kernel, compiled with the command line of __graft_entry__.build_aot (assembly instead
of a code object, so that the loop annotations of the compiler and the two assembler comments that mark the register-resident Newton loop
in the source survive): no vector-memory load between the entry of the Newton loop and its back edge, no VGPR spill, no scratch instruction."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "grid2op_amd", "csrc")
HEADLINE = ("step", "1,2,2,2,1,false,false,false")          # l2rpn_case14_sandbox, 4 096 lanes: two instances per wavefront
VMEM_LOAD = re.compile(r"^\s+(global_load|buffer_load|flat_load|scratch_load)")
SCRATCH = re.compile(r"^\s+scratch_")


def _blocks(asm):
    """[(label or None, annotation text, [instruction lines])] of the assembly, in layout order."""
    out = [(None, "", [])]
    lines = asm.split("\n")
    i = 0
    while i < len(lines):
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", lines[i])
        if m:
            note = m.group(2)
            while i + 1 < len(lines) and re.match(r"^\s+; ", lines[i + 1]) and "GPF_" not in lines[i + 1]:
                i += 1
                note += "\n" + lines[i]
            out.append((m.group(1)[2:], note, []))          # "BB0_465", as the annotations spell it
        else:
            out[-1][2].append(lines[i])
        i += 1
    return out


def newton_loop_lines(asm):
    """Instruction lines of every basic block of the register-resident Newton loop: the innermost loop around the back-edge marker, with
    the loops nested in it."""
    blocks = _blocks(asm)
    begin = [b for b in blocks if any("GPF_NEWTON_NWR_BEGIN" in l for l in b[2])]
    back = [b for b in blocks if any("GPF_NEWTON_NWR_BACKEDGE" in l for l in b[2])]
    assert len(begin) == 1 and len(back) == 1, "the markers of the Newton loop are not in the assembly (exactly once each)"
    label, note, _ = back[0]
    m = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
    header = m.group(1) if m else label                     # (the marker's block is the loop header itself)
    assert "Loop Header" in [b for b in blocks if b[0] == header][0][1], header
    body = [b for b in blocks if b[0] == header or re.search(r"Header=%s\b" % header, b[1]) or re.search(r"Parent Loop %s\b" % header, b[1])]
    assert begin[0] not in body, "the loop found contains its own entry marker"
    return [l for b in body for l in b[2]]


def _compile_headline(tmp_path, flags):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this host")
    objs = [o for o in ge.aot_objects() if (o[2], o[3]) == HEADLINE and o[4] == flags]
    assert len(objs) == 1, "the manifest no longer names the headline variant"
    hdr = objs[0][1]
    src = tmp_path / "k.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "gridpf_common.hpp"\n#include "gridpf_sparse.hpp"\nnamespace gpf {\n'
                   f"template __global__ void step_sparse_kernel<{HEADLINE[1]}>(const DevParamsS* __restrict__, const int* __restrict__, "
                   "const int* __restrict__, int, double, StepArgs);\n}\n")
    out = tmp_path / "k.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", *flags.split(), "-DGPF_JIT", "-include", hdr,
           f"-I{CSRC}", str(src), "-o", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    return out.read_text()


@pytest.mark.parametrize("flags", ["", "-fno-unroll-loops"])       # the two builds of the library's default policy (JIT_FLAG_SETS)
def test_newton_loop_of_the_headline_kernel_loads_nothing_from_global_memory(flags, tmp_path):
    asm = _compile_headline(tmp_path, flags)
    loop = newton_loop_lines(asm)
    # it IS the Newton loop: the LU's f64 LDS atomics and the sincos of the update phase are inside, and it is a real loop body
    assert sum("ds_add_f64" in l for l in loop) >= 12 and any("v_rndne_f64" in l or "v_fract_f64" in l or "v_sin_f32" in l for l in loop)
    assert len([l for l in loop if re.match(r"^\s+[a-z]", l)]) > 300
    loads = [l.strip() for l in loop if VMEM_LOAD.match(l)]
    assert not loads, f"vector-memory loads inside the Newton loop: {loads[:8]}"
    assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", asm).group(1)) == 0
    assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", asm).group(1)) == 0
    scratch = [l.strip() for l in asm.split("\n") if SCRATCH.match(l)]
    assert not scratch, scratch[:8]


def test_loop_finder_sees_a_load_when_there_is_one():
    """The checker on a hand-written listing: a load in a block of the marked loop (or of a loop nested in it) is found, one outside is not."""
    asm = "\n".join([
        "\tglobal_load_dword v1, v0, s[0:1]",
        "\t; GPF_NEWTON_NWR_BEGIN",
        ".LBB0_1:                                ; =>This Loop Header: Depth=1",
        "                                        ;     Child Loop BB0_2 Depth 2",
        "\tds_add_f64 v2, v[4:5]",
        ".LBB0_2:                                ;   Parent Loop BB0_1 Depth=1",
        "                                        ; =>  This Inner Loop Header: Depth=2",
        "\tglobal_load_dwordx2 v[6:7], v0, s[0:1]",
        "\ts_cbranch_execnz .LBB0_2",
        ".LBB0_3:                                ;   in Loop: Header=BB0_1 Depth=1",
        "\t; GPF_NEWTON_NWR_BACKEDGE",
        "\ts_cbranch_vccnz .LBB0_1",
        ".LBB0_4:",
        "\tbuffer_load_dword v8, v0, s[4:7], 0 offen",
    ])
    loop = newton_loop_lines(asm)
    assert [l.strip() for l in loop if VMEM_LOAD.match(l)] == ["global_load_dwordx2 v[6:7], v0, s[0:1]"]
    assert not VMEM_LOAD.match("\ts_buffer_load_dword s0, s[4:7], 0x0") and not VMEM_LOAD.match("\ts_load_dwordx2 s[0:1], s[2:3], 0x0")
