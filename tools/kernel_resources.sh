#!/bin/bash
# VGPRs / scratch / spills of every kernel instantiation of one translation unit (default: the step kernels)
#   tools/kernel_resources.sh aot     the ahead-of-time grid-specialised objects of grid2op_amd/aot/manifest.json instead (both flag sets;
#                                     a variant whose string ends in a number is the object of that launch-feature word)
if [ "$1" = aot ]; then
  cd "$(dirname "$0")/.." && exec python - <<'EOF'
import re, subprocess, tempfile, os
from concurrent.futures import ThreadPoolExecutor
import __graft_entry__ as ge
tmp = tempfile.mkdtemp(prefix="kres_")
def one(job):
    k, (_, hdr, kname, variant, flags) = job
    src = os.path.join(tmp, f"k{k}.hip")
    args = ("const DevParamsS* __restrict__, int, const int* __restrict__, const int* __restrict__, int, int, double" if kname == "runpf" else
            "const DevParamsS* __restrict__, const int* __restrict__, const int* __restrict__, int, double, StepArgs")
    open(src, "w").write('#include <hip/hip_runtime.h>\n#include "gridpf_common.hpp"\n#include "gridpf_sparse.hpp"\nnamespace gpf {\n'
                         f"template __global__ void {kname}_sparse_kernel<{variant}>({args});\n}}\n")
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--genco", *flags.split(), "-DGPF_JIT", "-include", hdr,
                        f"-I{ge.CSRC}", src, "-o", src[:-4] + ".co", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    g = lambda pat: (re.search(pat, p.stderr) or [None, "?"])[1]
    pats = dict(vgpr=r" VGPRs: (\d+)", sgpr=r"TotalSGPRs: (\d+)", scratch=r"ScratchSize \[bytes/lane\]: (\d+)", vgpr_spill=r"VGPRs Spill: (\d+)",
                sgpr_spill=r"SGPRs Spill: (\d+)")
    return f"{os.path.basename(hdr)} {kname}<{variant}> [{flags}] " + " ".join(f"{k_}={g(v_)}" for k_, v_ in pats.items())
jobs = [(k, o) for k, o in enumerate(ge.aot_objects()) if o[2] is not None]
with ThreadPoolExecutor(max_workers=8) as ex:
    for line in ex.map(one, jobs):
        print(line)
EOF
fi
unit=${1:-grid2op_amd/csrc/gridpf_launch_step.hip}
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $EXTRA -Rpass-analysis=kernel-resource-usage -c "$unit" -o /tmp/_kr.o 2>&1 |
  grep "remark:" | sed -E 's/.*remark: +//; s/ \[-Rpass.*//' |
  awk '/^Function Name/ {if (n) print n, v, sg, sc, sp; n=$3} /^VGPRs:/ {v="vgpr="$2} /^TotalSGPRs:/ {sg="sgpr="$2} /^ScratchSize/ {sc="scratch="$3} /^SGPRs Spill/ {sp="sgpr_spill="$3} END {print n, v, sg, sc, sp}' |
  sed -E 's/_ZN3gpf[0-9]+([a-z_]+)ILi([0-9])ELi([0-9])ELi([0-9])ELi([0-9])ELi([0-9])ELb([01])ELb([01])E[A-Za-z0-9_]* /\1<NB=\2,ST=\3,IPW=\4,MINW=\5,WPI=\6,TC=\7,YR=\8> /'
