#!/usr/bin/env python3
"""Register / scratch / LDS / occupancy table of every kernel of one csrc/*.hip file, as the compiler reports it
(-Rpass-analysis=kernel-resource-usage with the flags csrc/Makefile gives that file).  *(container)*
usage: tools/kernel_usage.py et_fit.hip [-DFLAG ...] [--grep substring]
       tools/kernel_usage.py et_kmeans.hip [-DFLAG ...] --digest [--csrc DIR]   name and sha256 of every device function's
           assembly and of every kernel's descriptor.  --csrc DIR compiles another checkout's csrc/ with THIS checkout's
           flags: `diff` the two outputs to prove that a change left the device code alone.  `all` for the file: every
           source of the Makefile, then et_kmeans.hip -DET_TEST_HOOKS"""
import hashlib
import os
import re
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eigentrajectory_amd", "csrc")


def ask_make(target):
    """csrc/Makefile is the one place that lists the sources and their flags"""
    return subprocess.run(["make", "-s", "-C", CSRC, target], stdout=subprocess.PIPE, text=True, check=True).stdout.split()


def flags_of(src):
    return ask_make("print-flags-" + os.path.splitext(os.path.basename(src))[0]) + ["--cuda-device-only"]


def digest(src, extra, csrc):
    """Per symbol, because emission order follows the host code.  Local labels carry the function's position in the file
    (.LBB13_2, .Lfunc_end13, .LJTI13_0; "Header=BB13_29" in the loop comments) or a file-wide count (.Ltmp57): that number is
    taken out, the rest stays."""
    asm = subprocess.run(["/opt/rocm/bin/hipcc"] + flags_of(src) + ["-S", "-o", "-"] + extra + [src], cwd=csrc, stdout=subprocess.PIPE,
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
    csrc = CSRC
    if "--csrc" in args:
        i = args.index("--csrc")
        csrc = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    if "--digest" in args:
        args.remove("--digest")
        if args[0] != "all":
            return digest(args[0], args[1:], csrc)
        for src, extra in [(s, []) for s in ask_make("print-srcs")] + [("et_kmeans.hip", ["-DET_TEST_HOOKS"])]:
            print("==", src, *extra, flush=True)
            digest(src, extra, csrc)
        return
    pat = None
    if "--grep" in args:
        i = args.index("--grep")
        pat = args[i + 1]
        del args[i:i + 2]
    src, extra = args[0], args[1:]
    out = subprocess.run(["/opt/rocm/bin/hipcc"] + flags_of(src) + ["-Rpass-analysis=kernel-resource-usage"] + extra + ["-c", src, "-o", "/dev/null"], cwd=csrc,
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
