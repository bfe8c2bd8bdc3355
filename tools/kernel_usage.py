#!/usr/bin/env python3
"""Register / scratch / LDS / occupancy table of every kernel of one csrc/*.hip file, as the compiler reports it
(-Rpass-analysis=kernel-resource-usage with the Makefile's flags).  *(container)*
usage: tools/kernel_usage.py et_fit.hip [-DFLAG ...] [--grep substring]
       tools/kernel_usage.py et_kmeans.hip [-DFLAG ...] --digest   name and sha256 of every device function's assembly and of
           every kernel's descriptor: `diff` the output of two checkouts to prove that a host-side change left the device code alone"""
import hashlib
import os
import re
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eigentrajectory_amd", "csrc")
FLAGS = ("--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -mllvm -amdgpu-mfma-vgpr-form=1 "
         "-fno-slp-vectorize --cuda-device-only -Rpass-analysis=kernel-resource-usage").split()


def digest(src, extra):
    """Per symbol, because emission order follows the host code.  Local labels carry the function's position in the file
    (.LBB13_2, .Lfunc_end13, .LJTI13_0; "Header=BB13_29" in the loop comments) or a file-wide count (.Ltmp57): that number is
    taken out, the rest stays."""
    flags = [f for f in FLAGS if not f.startswith("-Rpass")] + ["-S", "-o", "-"]
    asm = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + extra + [src], cwd=CSRC, stdout=subprocess.PIPE,
                         text=True, check=True).stdout  # (the compiler's diagnostics go to the terminal)
    bodies, cur = {}, None
    for line in asm.splitlines():
        if "__hip_cuid_" in line:
            continue
        if ".amdgpu_metadata" in line:  # (one list for the file, in emission order; the descriptors carry the same figures)
            break
        m = re.match(r"([A-Za-z_$][\w.$]*):|\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = bodies.setdefault(m.group(1) or m.group(2) + " (descriptor)", [])
        if cur is not None:
            cur.append(re.sub(r"(\.L|\b)(BB|func_begin|func_end|tmp|JTI)\d+", r"\1\2", line.strip()))
        if ".end_amdhsa_kernel" in line or line.startswith("\t.section"):
            cur = None
    for name in sorted(bodies):
        print(hashlib.sha256("\n".join(bodies[name]).encode()).hexdigest(), name)


def main():
    args = sys.argv[1:]
    if "--digest" in args:
        args.remove("--digest")
        return digest(args[0], args[1:])
    pat = None
    if "--grep" in args:
        i = args.index("--grep")
        pat = args[i + 1]
        del args[i:i + 2]
    src, extra = args[0], args[1:]
    out = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + extra + ["-c", src, "-o", "/dev/null"], cwd=CSRC,
                         stderr=subprocess.PIPE, text=True).stderr
    rows, cur = [], {}
    for line in out.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m and "error" in line:
            print(line)
        if not m:
            continue
        key, val = m.group(1).split()[0], m.group(2)
        if key == "Function":
            cur = dict(name=val)
            rows.append(cur)
        else:
            cur[key] = val
    names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    print(f"{'vgpr':>5}{'agpr':>5}{'scratch':>8}{'occ':>4}{'lds':>7}  kernel")
    for r, n in zip(rows, names):
        n = re.sub(r"\(.*", "", n).replace("void ", "")
        if pat and pat not in n:
            continue
        print(f"{r.get('VGPRs', '?'):>5}{r.get('AGPRs', '?'):>5}{r.get('ScratchSize', '?'):>8}{r.get('Occupancy', '?'):>4}{r.get('LDS', '?'):>7}  {n}")


if __name__ == "__main__":
    main()
