"""CPU check on the ISA of the observation gather kernel (grid2op_amd/csrc/gridpf_obs.hpp), compiled for gfx950 with the library's command
line: the segment table comes through scalar loads, float sources move 16 bytes per lane where aligned, nothing goes to scratch (SGPRs the
register file cannot hold are parked in VGPR lanes, not in memory) and no LDS is used.  And the chronics row index is ONE function, shared
by the step kernel (K9) and the observation clock -- a source edit of the step kernel that leaves its instructions alone: the per-kernel
digests of the step / runpf instruction streams (tools/kernel_isa_digest.py) taken on the commit before it and on this tree are both in
profiles/, equal line for line, and the grid-specialised headline variants are compiled again here and compared with that record."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "grid2op_amd", "csrc")


def test_gather_kernel_uses_scalar_loads_wide_accesses_and_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this host")
    out = tmp_path / "obs.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", os.path.join(CSRC, "gridpf_capi_obs.hip"), "-o", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    asm = out.read_text()
    body = asm[asm.index("obs_gather_kernel"):]
    assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", asm).group(1)) == 0
    assert int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", asm).group(1)) == 0
    assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", asm).group(1)) == 0
    assert not [l for l in body.split("\n") if re.match(r"^\s+scratch_", l)]
    assert len([l for l in body.split("\n") if re.match(r"^\s+s_load_dword", l)]) >= 5          # segment fields + row scalars
    assert any("global_load_dwordx4" in l for l in body.split("\n")) and any("global_store_dwordx4" in l for l in body.split("\n"))
    assert not [l for l in body.split("\n") if re.match(r"^\s+(global|flat|buffer|ds)_atomic|^\s+ds_", l)]


def test_one_chronics_row_index_function():
    common = open(os.path.join(CSRC, "gridpf_common.hpp")).read()
    assert len(re.findall(r"int chron_row_index\(", common)) == 1
    assert "chron_row_index(sa.t, off, sa.T)" in open(os.path.join(CSRC, "gridpf_sparse.hpp")).read()
    assert "chron_row_index(" in open(os.path.join(CSRC, "gridpf_obs.hpp")).read()


def _record(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        return [l.rstrip("\n") for l in f if l.strip()]


def test_step_and_runpf_digests_before_and_after_are_equal_and_cover_every_variant():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    before, after = _record("step_runpf_isa_digest_parent.txt"), _record("step_runpf_isa_digest.txt")
    assert before == after and before[0].startswith("# compiler:")
    body = after[1:]
    assert all(re.search(r"  \d+ lines  [0-9a-f]{64}$", l) and int(re.search(r"  (\d+) lines", l).group(1)) > 100 for l in body)
    for unit, kernel in (("gridpf_launch_step.hip", "step_sparse_kernel"), ("gridpf_launch_runpf.hip", "runpf_sparse_kernel")):
        assert len([l for l in body if l.startswith(unit + "  ") and kernel in l]) >= 4, unit        # the generic template instantiations
    aot = [o for o in ge.aot_objects() if o[2] is not None]
    assert {o[2] for o in aot} == {"step", "runpf"}
    for _, hdr, kname, variant, flags in aot:                       # every ahead-of-time variant, both flag sets
        tag = "aot %s <%s> [%s] %s  " % (os.path.basename(hdr), variant, flags, kname)
        assert len([l for l in body if l.startswith(tag)]) == 1, tag


@pytest.mark.parametrize("which", ["step:1,2,2,2,1,false,false,false", "runpf:1,2,2,2,1,false,false"])     # the 14-substation headline pair
def test_headline_variants_compile_to_the_recorded_instruction_streams(which):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this host")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_digest
    got = kernel_isa_digest.digest_lines(ROOT, only_aot=which, jobs=2)
    rec = _record("step_runpf_isa_digest.txt")
    assert len(got) == 3                            # the compiler line + the variant under the two flag sets
    if got[0] != rec[0]:
        return                                  # another compiler than the record's: its digests say nothing about the source
    assert all(l in rec for l in got[1:]), got
