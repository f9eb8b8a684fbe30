"""One line per step / runpf kernel: a SHA-256 of its gfx950 instruction stream (developer tool; CPU only, needs hipcc).

A change that must leave the step and runpf kernels alone is checked by running this on the commit before and on the commit after and
comparing the two listings (profiles/step_runpf_isa_digest.txt is the listing of this tree).  Covered: every kernel of the two launch units
the library is built from (gridpf_launch_step.hip, gridpf_launch_runpf.hip: all template instantiations) and every ahead-of-time
grid-specialised variant of grid2op_amd/aot/manifest.json under both flag sets of the library's policy, each compiled with the command line
`__graft_entry__` uses, to assembly instead of an object.  Hashed per kernel: the lines between its label and its end label, without
comments, blank lines and assembler directives -- instructions and local labels only, so the compilation-unit id symbol, debug notes and
metadata do not enter.

    python tools/kernel_isa_digest.py [--root CHECKOUT] [--out FILE] [--only-aot step:1,2,2,2,1,false,false,false]

--units 'gridpf_capi*.hip' lists the kernels of those units of grid2op_amd/csrc instead (no ahead-of-time variants): a change that moves
kernels between units leaves every kernel's digest and line count as it was, in exactly one unit (local labels are hashed without the
function's index in its unit).
"""
import argparse
import glob
import hashlib
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

UNITS = ("gridpf_launch_step.hip", "gridpf_launch_runpf.hip")


def kernel_digests(asm, movable=False):
    """{kernel symbol: sha256 of its instruction lines} of one assembly listing (functions of type @function that are kernels or not:
    every `.type NAME,@function` body up to its `.Lfunc_end`).  movable: local labels lose the function's index in its unit (.LBB4_3 ->
    .LBB_3), so that a kernel keeps its digest when it moves to another unit."""
    out = {}
    lines = asm.split("\n")
    i = 0
    while i < len(lines):
        m = re.match(r"^\s*\.type\s+([A-Za-z0-9_.$]+),@function", lines[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        while i < len(lines) and not lines[i].startswith(name + ":"):
            i += 1
        h = hashlib.sha256()
        n = 0
        i += 1
        while i < len(lines) and not re.match(r"^\.Lfunc_end\d+:", lines[i]):
            l = lines[i].split(";")[0].rstrip()
            if movable:
                l = re.sub(r"(\.L[A-Za-z_]+)\d+_(\d+)", r"\1_\2", l)
            if l.strip() and not re.match(r"^\s+\.", l):           # instructions and labels; no directives
                h.update(l.strip().encode() + b"\n")
                n += 1
            i += 1
        out[name] = (h.hexdigest(), n)
    return out


def _asm(cmd, out):
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit("%s\n%s" % (" ".join(cmd), p.stderr[-3000:]))
    with open(out) as f:
        return f.read()


def digest_lines(root, only_aot=None, jobs=8, units=None):
    csrc = os.path.join(root, "grid2op_amd", "csrc")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    spec = importlib.util.spec_from_file_location("_ge_digest", os.path.join(root, "__graft_entry__.py"))
    ge = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ge)
    base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S"]
    tmp = tempfile.mkdtemp(prefix="isa_digest_")
    work = []
    if only_aot is None:
        for u in UNITS if units is None else sorted(os.path.basename(f) for f in glob.glob(os.path.join(csrc, units))):
            work.append((u, base + ["-fPIC", os.path.join(csrc, u), "-o", os.path.join(tmp, u + ".s")], os.path.join(tmp, u + ".s")))
    for k, (_, hdr, kname, variant, flags) in enumerate([] if units else ge.aot_objects()):
        if kname is None or (only_aot is not None and f"{kname}:{variant}" != only_aot):
            continue
        src = os.path.join(tmp, f"aot{k}.hip")
        if kname == "runpf":
            decl = (f"runpf_sparse_kernel<{variant}>(const DevParamsS* __restrict__, int, const int* __restrict__, const int* __restrict__, "
                    "int, int, double)")
        else:
            decl = (f"step_sparse_kernel<{variant}>(const DevParamsS* __restrict__, const int* __restrict__, const int* __restrict__, int, "
                    "double, StepArgs)")
        with open(src, "w") as f:
            f.write('#include <hip/hip_runtime.h>\n#include "gridpf_common.hpp"\n#include "gridpf_sparse.hpp"\nnamespace gpf {\n'
                    f"template __global__ void {decl};\n}}\n")
        tag = "aot %s <%s> [%s] %s" % (os.path.basename(hdr), variant, flags, kname)
        work.append((tag, base + flags.split() + ["-DGPF_JIT", "-include", hdr, f"-I{csrc}", src, "-o", src[:-4] + ".s"], src[:-4] + ".s"))
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        asms = list(ex.map(lambda w: _asm(w[1], w[2]), work))
    ver = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout
    m = re.search(r"clang version [^\n]*", ver)
    lines = ["# compiler: " + (m.group(0).strip() if m else "unknown")]
    for (tag, _, _), asm in zip(work, asms):
        for name, (dig, n) in sorted(kernel_digests(asm, units is not None).items()):
            lines.append(f"{tag}  {name}  {n} lines  {dig}")
    shutil.rmtree(tmp, ignore_errors=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-aot", default=None)
    ap.add_argument("--units", default=None)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    text = "\n".join(digest_lines(os.path.abspath(a.root), a.only_aot, a.jobs, a.units)) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
