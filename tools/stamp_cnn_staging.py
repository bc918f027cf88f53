#!/usr/bin/env python3
"""Diagnostic build of the band CNN: where does a wavefront WAIT for the input staging?

Patches a copy of llicti_amd/csrc into build/stamp_cnn_src (the product source has no stamp) and builds build/lib_stamp_cnn.so: every
wavefront of a few workgroups of head 0 stamps, with s_memtime, per tile

  stage     cycles inside its stage_next site (address arithmetic + issue of its 3 / 6 / 9 LDS-DMA instructions: a blocked vector-memory
            issue path shows here),
  drain_ld  cycles in the drain in front of the barrier until the wave's LDS-DMA has landed,
  drain_st  ... until its params stores are acknowledged as well (--stores-last only: a source whose eight params stores are the last
            vector-memory instructions in front of the drain, so that a counted vmcnt(8) separates the two; full tiles only),
  barrier   cycles in the s_barrier behind the drain,
  tile      barrier to barrier.

and prints the per-tile means at the end of the kernel (launches of >= 8 tiles per workgroup; the first tile of a workgroup, whose drain
also waits for the weight pack, is not counted).  A wave's drain is hidden behind its barrier wait unless it is the LAST to arrive: what a
tile pays is the drain of the wave with the smallest barrier wait.

  here:     python tools/stamp_cnn_staging.py [--stores-last]
  GPU box:  LLICTI_HIP_SO=$PWD/build/lib_stamp_cnn.so python tools/bench_cnn.py > log;  python tools/stamp_cnn_staging.py --summarise log out.json

Read the SHARES, not the run time: the stamps' own waits (s_memtime returns through lgkmcnt) forbid overlaps the product kernel has."""
import json
import os
import re
import shutil
import statistics
import subprocess
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summarise(log, out):
    pat = re.compile(r"CNNSTAMP band (\d) th (\d+) wg (\d+) wave (\d+) tiles (\d+) stage (\d+) drain_ld (\d+) drain_st (\d+) barrier (\d+) tile (\d+)")
    rows = [tuple(int(x) for x in m.groups()) for m in map(pat.search, open(log)) if m]
    res = {"what": "s_memtime stamps of band_params_kernel (tools/stamp_cnn_staging.py), tools/bench_cnn.py, level-0 launches (the ones with >= 8 tiles "
                   "per workgroup): median over launches and workgroups of the per-tile mean cycles of a wave; group g = waves 4g .. 4g+3 (staging site 3 - g; site g in builds older than the reversed site order)",
           "bands": {}}
    for band in sorted({r[0] for r in rows}):
        sel = [r for r in rows if r[0] == band and r[1] == 16]
        groups = {}
        for g in range(4):
            gs = [r for r in sel if r[3] // 4 == g]
            if gs:
                groups[f"group{g}"] = {k: statistics.median(r[i] for r in gs) for k, i in
                                       (("stage", 5), ("drain_ld", 6), ("drain_st", 7), ("barrier", 8), ("tile", 9))}
        # the wave that arrives last at the barrier (smallest barrier wait) of every (launch, workgroup) sample: its drain is exposed
        # (a launch's lines arrive in any order: the k-th line of a (workgroup, wave) belongs to the k-th launch)
        seen, samples = {}, {}
        for r in sel:
            k = seen[(r[2], r[3])] = seen.get((r[2], r[3]), -1) + 1
            samples.setdefault((k, r[2]), []).append(r)
        last = [min(ws, key=lambda r: r[8]) for ws in samples.values() if len(ws) == 16]
        if last:
            groups["last_arriver"] = {k: statistics.median(r[i] for r in last) for k, i in
                                      (("stage", 5), ("drain_ld", 6), ("drain_st", 7), ("barrier", 8), ("tile", 9))}
            groups["last_arriver"]["samples"] = len(last)
        res["bands"][str(band)] = groups
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if len(sys.argv) > 1 and sys.argv[1] == "--summarise":
    summarise(sys.argv[2], sys.argv[3])
    sys.exit(0)

stores_last = "--stores-last" in sys.argv
work = os.path.join(root, "build", "stamp_cnn_src")
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
    "    int cur = 0;\n    unsigned long long TT[5] = { 0, 0, 0, 0, 0 }, t_tile = 0; int ntile = 0, st_full = 0;\n")
drain = '        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");\n        __syncthreads();\n'
rep(drain,
    f"        const unsigned long long d0 = {NOW};\n"
    + ('        if (st_full) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");\n' if stores_last else "")
    + f"        const unsigned long long d1 = {NOW};\n"
    + '        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");\n'
    + f"        const unsigned long long d2 = {NOW};\n"
    + "        __syncthreads();\n"
    + f"        const unsigned long long d3 = {NOW};\n"
    + "        if (t_tile) { " + ("if (st_full) { TT[1] += d1 - d0; TT[2] += d2 - d1; } else TT[1] += d2 - d0;" if stores_last else "TT[1] += d2 - d0;")
    + " TT[3] += d3 - d2; TT[4] += d3 - t_tile; ++ntile; }\n"
    + "        t_tile = d3;\n"
    + "        st_full = (ty + 1) * kTileH <= (RAGGED ? gv[img].h : g.h) && (tx + 1) * kTileW <= (RAGGED ? gv[img].w : g.w);\n")
rep("            if (more && stage_site == site % CNN_STAGE_SITES) stage(tile + gridDim.x, lds_in + (cur ^ 1) * (NPL * kInPlane));\n",
    "            if (more && stage_site == site % CNN_STAGE_SITES) {\n"
    f"                const unsigned long long s0 = {NOW};\n"
    "                stage(tile + gridDim.x, lds_in + (cur ^ 1) * (NPL * kInPlane));\n"
    f"                const unsigned long long s1 = {NOW};\n"
    "                if (t_tile) TT[0] += s1 - s0;\n"
    "            }\n")
# the print goes behind the tile loop: the loop's closing brace is the first "\n    }\n" after "cur ^= 1;"
i = s.index("        cur ^= 1;\n")
j = s.index("\n    }\n", i) + 7
s = s[:j] + ('    if (ntile >= 7 && blockIdx.y == 0 && (blockIdx.x & 63) == 0 && lane == 0)\n'
             '        printf("CNNSTAMP band %d th %d wg %d wave %d tiles %d stage %llu drain_ld %llu drain_st %llu barrier %llu tile %llu\\n", BAND, TH, (int)blockIdx.x, wave, ntile,\n'
             '               TT[0] / ntile, TT[1] / ntile, TT[2] / ntile, TT[3] / ntile, TT[4] / ntile);\n') + s[j:]
open(os.path.join(work, "band_cnn.hpp"), "w").write(s)
so = os.path.join(root, "build", "lib_stamp_cnn.so")
subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                       "-Wno-unused-value", "-o", so, os.path.join(work, "llicti_hip.hip")])
print("built", os.path.relpath(so, root))
