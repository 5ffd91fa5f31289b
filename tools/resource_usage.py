#!/usr/bin/env python3
"""Register / scratch / LDS table of the kernels: hipcc -Rpass-analysis=kernel-resource-usage with the Makefile's flags, one line per
kernel, sorted by name.  All ten template parameters of conv_stream_kernel are decoded, and its LDS column is the dynamic size the
launcher asks for (conv.hip: stream_lds / x3_stream_lds, restated below; conv.hip holds its own seven values to literals in a
static_assert, which the table can be read against); every other kernel's is the static size the compiler reports.
Usage: python tools/resource_usage.py [--csrc DIR] [conv.hip stem.hip post.hip ...] [-- extra hipcc flags]   (default: conv.hip)"""
import re, subprocess, sys, os, tempfile
argv = sys.argv[1:]
extra = argv[argv.index("--") + 1:] if "--" in argv else []
argv = argv[:argv.index("--")] if "--" in argv else argv
csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vnect_amd", "csrc")
if "--csrc" in argv:
    csrc = argv[argv.index("--csrc") + 1]
    del argv[argv.index("--csrc"):argv.index("--csrc") + 2]
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]


def stream_lds(bm, bn, kg, ns, x3):  # conv.hip: stream_lds, x3_stream_lds
    ring = ns * (bm * 32 + bn * 48) * kg * 4 if x3 else ns * (bm + bn) * 32 * kg * 4
    return ring + ((kg - 1) * (4 // kg) * (3 if bn == 96 and not x3 else 1) * 4096 + 64 if kg > 1 else 0)


def table(name):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["/opt/rocm/bin/hipcc"] + FLAGS + ([] if name == "conv.hip" else ["-ffp-contract=off"]) + ["-Rpass-analysis=kernel-resource-usage"]
        out = subprocess.run(cmd + extra + ["-c", name, "-o", os.path.join(tmp, "ru.o")], cwd=csrc, capture_output=True, text=True).stderr
    cur, rows = None, {}
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1); rows[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/\w+\])?: (\d+)", line)
        if m and cur: rows[cur][m.group(1).strip()] = int(m.group(2))
    if not rows: sys.exit(out)
    print("# %s: %d kernels" % (name, len(rows)))
    print("%-78s %5s %5s %7s %6s %6s %7s" % ("kernel", "VGPR", "SGPR", "scratch", "sspill", "vspill", "LDS"))
    for k, v in sorted(rows.items()):
        m = re.search(r"conv_stream_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d)ELi(\d)ELi(\d)ELb(\d)ELb(\d)ELb(\d)E", k)
        lds = v.get("LDS Size", -1)
        if m:
            p = [int(x) for x in m.groups()]
            k, lds = "stream<%d,%d,%d,%d,el%d,prof%d,fuse%d,span%d,x3%d,one%d>" % tuple(p), stream_lds(p[0], p[1], p[2], p[3], p[8])
        print("%-78s %5d %5d %7d %6d %6d %7d" % (k, v.get("VGPRs", -1), v.get("TotalSGPRs", -1), v.get("ScratchSize", -1), v.get("SGPRs Spill", -1), v.get("VGPRs Spill", -1), lds))


for f in argv or ["conv.hip"]:
    table(f)
