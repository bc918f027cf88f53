#!/usr/bin/env python3
"""Diagnostic build of the band CNN: which part of the tile do a wavefront's cycles go to?  (Round 9: the regions the tile ladder's variants
removed -- profiles/r9/cnn_tile_ladder.json -- stamped in the kernel that has them.)

Patches a copy of llicti_amd/csrc into build/stamp_cnn_phases_src (the product source has no stamp) and builds build/lib_stamp_cnn_phases<tag>.so:
every wavefront of a few workgroups of head 0 stamps, with s_memtime, per tile

  layer0    barrier -> the last MFMA of layer 0 issued (with the staging site behind the barrier),
  handoff   the remainder path's ReLU, its 16 ds_bpermute and their selects (config A only),
  relu0     staging site 1 and the ReLU of layer 0's 40 accumulator registers,
  layers12  layers 1 and 2 with their ReLUs, bias loads and staging sites 2 and 3,
  epilogue  the params stores' address arithmetic and issue,
  barrier   the drain and the s_barrier behind it,
  tile      barrier to barrier,

and prints the per-tile means at the end of the kernel (launches of >= 8 tiles per workgroup; a workgroup's first tile is not counted).

  here:     python tools/stamp_cnn_phases.py [tag] [extra hipcc flags, e.g. -DCNN_RELU_MED3=0]
  GPU box:  LLICTI_HIP_SO=$PWD/build/lib_stamp_cnn_phases<tag>.so python tools/bench_cnn.py > log;  python tools/stamp_cnn_phases.py --summarise log out.json

Read the SHARES and the DIFFERENCES between two stamped builds, not the run time: the stamps' own waits (s_memtime returns through lgkmcnt)
forbid overlaps the product kernel has."""
import json
import os
import re
import shutil
import statistics
import subprocess
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHASES = ("layer0", "handoff", "relu0", "layers12", "epilogue", "barrier", "tile")


def summarise(log, out):
    pat = re.compile(r"CNNPHASE band (\d) th (\d+) wg (\d+) wave (\d+) tiles (\d+) " + " ".join(p + r" (\d+)" for p in PHASES))
    rows = [tuple(int(x) for x in m.groups()) for m in map(pat.search, open(log)) if m]
    res = {"what": "s_memtime stamps of band_params_kernel (tools/stamp_cnn_phases.py), tools/bench_cnn.py, 16-row launches with >= 8 tiles per workgroup: "
                   "median over launches and workgroups of the per-tile mean cycles of a wave; group g = waves 4g .. 4g+3 (staging site 3 - g)",
           "bands": {}}
    for band in sorted({r[0] for r in rows}):
        sel = [r for r in rows if r[0] == band and r[1] == 16]
        groups = {}
        for g in range(4):
            gs = [r for r in sel if r[3] // 4 == g]
            if gs:
                groups[f"group{g}"] = {p: statistics.median(r[5 + i] for r in gs) for i, p in enumerate(PHASES)}
        if sel:
            groups["all_waves"] = {p: statistics.median(r[5 + i] for r in sel) for i, p in enumerate(PHASES)}
            groups["all_waves"]["samples"] = len(sel)
        res["bands"][str(band)] = groups
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if len(sys.argv) > 1 and sys.argv[1] == "--summarise":
    summarise(sys.argv[2], sys.argv[3])
    sys.exit(0)

tag = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else ""
extra = [a for a in sys.argv[1:] if a.startswith("-")]
work = os.path.join(root, "build", "stamp_cnn_phases_src")
shutil.rmtree(work, ignore_errors=True)
shutil.copytree(os.path.join(root, "llicti_amd", "csrc"), work)
main = open(os.path.join(work, "llicti_hip.hip")).read().replace('#include "../../include/llicti_hip.h"', f'#include "{root}/include/llicti_hip.h"')
open(os.path.join(work, "llicti_hip.hip"), "w").write(main)
s = open(os.path.join(work, "band_cnn.hpp")).read()


def rep(a, b):
    global s
    assert s.count(a) == 1, a
    s = s.replace(a, b, 1)


NOW = "__builtin_amdgcn_s_memtime()"
rep("    int cur = 0;\n",
    "    int cur = 0;\n    unsigned long long TT[7] = { 0, 0, 0, 0, 0, 0, 0 }, t_tile = 0, p_end = 0; int ntile = 0;\n")
rep('        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");\n        __syncthreads();\n',
    '        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");\n        __syncthreads();\n'
    f"        const unsigned long long p0 = {NOW};\n"
    "        if (t_tile) { TT[5] += p0 - p_end; TT[6] += p0 - t_tile; ++ntile; }\n")
rep("            if constexpr (kRem) {\n            dR = relu4(dR);\n",
    f"            pa = {NOW};\n            if constexpr (kRem) {{\n            dR = relu4(dR);\n")
rep("        f32x4 a0[kMT][kNT];\n", "        f32x4 a0[kMT][kNT];\n        unsigned long long pa = 0;\n")
rep("        if constexpr (CNN_STAGE_SITES > 1) stage_next(1);\n",
    f"        const unsigned long long p1 = {NOW};\n        if (!pa) pa = p1;\n        if constexpr (CNN_STAGE_SITES > 1) stage_next(1);\n")
rep("        // ---- layers 1 and 2, interleaved per 16-channel tile",
    f"        const unsigned long long p2 = {NOW};\n        // ---- layers 1 and 2, interleaved per 16-channel tile")
rep("        int store = 1;\n", f"        const unsigned long long p3 = {NOW};\n        int store = 1;\n")
rep("        cur ^= 1;\n",
    f"        p_end = {NOW};\n"
    "        if (t_tile) { TT[0] += pa - p0; TT[1] += p1 - pa; TT[2] += p2 - p1; TT[3] += p3 - p2; TT[4] += p_end - p3; }\n"
    "        t_tile = p0;\n"
    "        cur ^= 1;\n")
i = s.index("        cur ^= 1;\n")
j = s.index("\n    }\n", i) + 7
s = s[:j] + ('    if (ntile >= 7 && blockIdx.y == 0 && (blockIdx.x & 63) == 0 && lane == 0)\n'
             '        printf("CNNPHASE band %d th %d wg %d wave %d tiles %d ' + " ".join(p + " %llu" for p in PHASES) + '\\n", BAND, TH, (int)blockIdx.x, wave, ntile,\n'
             '               ' + ", ".join(f"TT[{k}] / ntile" for k in range(7)) + ");\n") + s[j:]
open(os.path.join(work, "band_cnn.hpp"), "w").write(s)
so = os.path.join(root, "build", f"lib_stamp_cnn_phases{tag}.so")
subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                       "-Wno-unused-value"] + extra + ["-o", so, os.path.join(work, "llicti_hip.hip")])
print("built", os.path.relpath(so, root))
