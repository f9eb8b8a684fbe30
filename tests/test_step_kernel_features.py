"""Launch features of the grid-specialised step kernel (gridpf_common.hpp: FEAT_*): the 14-substation headline kernel compiled for the
headline launch's feature word carries the launch's answers as literals, so its step loop is shorter and asks the parameter block less.

CPU checks on the ISA, with the command line and the loop finder of tests/test_step_kernel_words_resident.py: the feature build against the
grid-only build of the same variant -- no spill, no scratch, not more VGPRs, strictly fewer instructions and strictly fewer scalar loads
inside the step loop, still no vector-memory load in the marked Newton loop.  And the word in the manifest is the one the library computes
for the bench's headline launch (header-only handle, no GPU)."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT
from test_step_kernel_words_resident import CSRC, HEADLINE, SCRATCH, VMEM_LOAD, _blocks, newton_loop_lines

MANIFEST = os.path.join(ROOT, "grid2op_amd", "aot", "manifest.json")
INSTR = re.compile(r"^\s+[a-z]")
SLOAD = re.compile(r"^\s+s_(buffer_)?load_dword")


def headline_feature_variant():
    man = json.load(open(MANIFEST))
    ent = [e for e in man.values() if "l2rpn_case14_sandbox" in e["grids"]][0]
    feat = [v for k, v in ent["variants"] if k == "step" and v.startswith(HEADLINE[1] + ",")]
    assert len(feat) == 1, "the manifest names exactly one feature variant of the headline kernel"
    return os.path.join(ROOT, "grid2op_amd", "aot", ent["header"]), feat[0]


def step_loop_lines(asm):
    """Instruction lines of the step loop: the outermost loop around the marked Newton loop, with everything nested in it."""
    blocks = _blocks(asm)
    back = [b for b in blocks if any("GPF_NEWTON_NWR_BACKEDGE" in l for l in b[2])]
    assert len(back) == 1
    label, note, _ = back[0]
    m = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
    inner = m.group(1) if m else label                       # header of the Newton loop: its annotation names the loops around it
    note_h = [b for b in blocks if b[0] == inner][0][1]
    m = re.search(r"Parent Loop (BB\d+_\d+) Depth=1\b", note_h)
    assert m, "the Newton loop is not nested in a loop"
    header = m.group(1)
    assert "Loop Header: Depth=1" in [b for b in blocks if b[0] == header][0][1], header
    # a block names its innermost loop only; a loop header names every loop around it
    headers = {header} | {b[0] for b in blocks if "Loop Header" in b[1] and re.search(r"Parent Loop %s\b" % header, b[1])}
    body = [b for b in blocks if b[0] in headers or (re.search(r"in Loop: Header=(BB\d+_\d+)", b[1]) or [None, None])[1] in headers]
    assert back[0] in body
    return [l for b in body for l in b[2]]


def _compile(tmp_path, hdr, variant, tag):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this host")
    src = tmp_path / f"{tag}.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "gridpf_common.hpp"\n#include "gridpf_sparse.hpp"\nnamespace gpf {\n'
                   f"template __global__ void step_sparse_kernel<{variant}>(const DevParamsS* __restrict__, const int* __restrict__, "
                   "const int* __restrict__, int, double, StepArgs);\n}\n")
    out = tmp_path / f"{tag}.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-DGPF_JIT", "-include", hdr, f"-I{CSRC}", str(src),
           "-o", str(out)]
    return subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), out


def test_feature_build_of_the_headline_kernel_has_a_shorter_step_loop(tmp_path):
    hdr, variant = headline_feature_variant()
    jobs = [_compile(tmp_path, hdr, HEADLINE[1], "grid"), _compile(tmp_path, hdr, variant, "feat")]     # (side by side: a minute each)
    asm = []
    for p, out in jobs:
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-2000:]
        asm.append(out.read_text())
    grid, feat = asm
    num = lambda key, a: int(re.search(r"\.%s:\s*(\d+)" % key, a).group(1))  # noqa: E731
    assert num("vgpr_spill_count", feat) == 0 and num("private_segment_fixed_size", feat) == 0
    assert not [l for l in feat.split("\n") if SCRATCH.match(l)]
    assert num("vgpr_count", feat) <= num("vgpr_count", grid), (num("vgpr_count", feat), num("vgpr_count", grid))
    lg, lf = step_loop_lines(grid), step_loop_lines(feat)
    n_g, n_f = sum(bool(INSTR.match(l)) for l in lg), sum(bool(INSTR.match(l)) for l in lf)
    s_g, s_f = sum(bool(SLOAD.match(l)) for l in lg), sum(bool(SLOAD.match(l)) for l in lf)
    print(f"step loop: instructions {n_g} -> {n_f}, scalar loads {s_g} -> {s_f}; VGPRs {num('vgpr_count', grid)} -> {num('vgpr_count', feat)}")
    assert n_g > 3000, "the loop found is not the step loop"
    assert n_f < n_g and s_f < s_g, (n_g, n_f, s_g, s_f)
    newton = newton_loop_lines(feat)
    assert sum("ds_add_f64" in l for l in newton) >= 12 and len([l for l in newton if INSTR.match(l)]) > 300
    assert not [l.strip() for l in newton if VMEM_LOAD.match(l)]


def test_host_word_function_table_under_sanitizers(tmp_path):
    """tests/native/step_features_main.cpp: a stand-alone host program (its own main) around gpf_step_features, built with
    the address and undefined-behaviour sanitizers on the HOST side only (no device code is compiled) -- every bit has a launch
    description that clears it, the headline description sets them all."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this host")
    exe = tmp_path / "step_features"
    host_san = "-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined".split()     # host compilation only
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", *host_san,
           os.path.join(ROOT, "tests", "native", "step_features_main.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok:") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-2000:])


def test_manifest_word_is_the_word_of_the_bench_headline_launch(load_model):
    """bench.py's headline: 4 096 lanes of l2rpn_case14_sandbox, load jitter, rebalance = 1.02, no cascade, 16-step launches with the
    observation trajectory on.  The manifest's word was written by `python -m grid2op_amd.aot ... --features headline`; the library says the
    same for that launch, and a launch that differs in any one feature gets another word."""
    sys.path.insert(0, ROOT)
    from grid2op_amd import aot
    from grid2op_amd.engine import PowerFlowEngine
    _, variant = headline_feature_variant()
    word = int(variant.split(",")[8])
    eng = PowerFlowEngine(load_model("l2rpn_case14_sandbox"), n_lanes=4096, device=-1)
    try:
        head = dict(n_steps=16, lane_scale=True, trajectory_obs=True, rebalance=1.02)
        assert aot.FEATURE_LAUNCHES["headline"] == head
        assert eng.feature_word(**head) == word
        assert eng.feature_word(**dict(head, n_steps=20)) == word and eng.feature_word(**dict(head, rebalance=1.05)) == word
        others = [dict(head, cascade=True), dict(head, auto_reset=True), dict(head, outages=True), dict(head, trajectory_obs=False),
                  dict(head, n_steps=1), dict(head, is_dc=True), dict(head, lane_scale=False), dict(head, rebalance=0.0), dict(head, gen_delta=True),
                  dict(head, warm_start=True), dict(head, nb_ts_reco=10)]
        got = [eng.feature_word(**o) for o in others]
        assert all(w != word and (w & ~word) == 0 for w in got), got          # the headline launch makes every assumption there is
        assert len(set(got)) == len(got)
    finally:
        eng.close()
    _, variants = aot.header_and_variants(load_model("l2rpn_case14_sandbox"), [4096], features=["headline"])
    assert ["step", variant] in variants
