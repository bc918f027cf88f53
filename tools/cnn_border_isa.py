#!/usr/bin/env python3
"""What does staging a BORDER tile of the band CNN cost, in instructions per 64-float piece?  Count from the device assembly (no GPU needed).

    python tools/cnn_border_isa.py [--asm llicti.s] [--json out.json] [kernel-name substring ...]

Without --asm the tool compiles llicti_hip.hip itself, with -DCNN_STAGE_FAST=0: in that build no tile takes the interior fast path, so
every staging instruction of the tile loop belongs to the border path and nothing has to be told apart.  (The product build is what
tools/cnn_wait_audit.py and tools/kernel_resources.py look at.)

Per band_params*_kernel instantiation the tile loop is cut into basic blocks.  STAGING blocks are the ones with no matrix, LDS, barrier or
store instruction; connected over the branches between them they form one group per staging site (the sites are separated by MFMA code).
Per site:
    pieces      LDS-DMA requests outside a rolled inner loop (the unrolled pieces of a wave; 0 where the path is a rolled loop only)
    straight    instructions of the site outside the rolled loop: tile -> (image, row, column), the per-tile set-up, the unrolled pieces
    loop        instructions of one pass through the rolled loop (one piece by the general, clamping formula), vector / scalar / DMA
and the figure to compare builds by:
    per_piece   straight / pieces                 where the pieces are unrolled (the set-up is counted in: an upper bound for a tile
                                                  whose pieces all take the unrolled form);
                loop + straight / pieces-of-a-wave where every piece goes through the rolled loop.
The table has the largest site of each instantiation.  parse() is what tests/test_cnn_border_isa_cpu.py asserts through."""
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cnn_wait_audit                                    # noqa: E402
from kernel_resources import FLAGS, SRC                  # noqa: E402

_TPL = re.compile(r"band_params\w*_kernelILi(\d)ELi(\d+)ELb([01])E")
_NOT_STAGING = re.compile(r"^(v_mfma|ds_|s_barrier|global_store|buffer_store|flat_store|s_setprio|s_endpgm)")


def wave_pieces(name):
    """pieces a wave stages per tile, from the template arguments in the mangled name (band, tile rows)"""
    band, th, _ = (int(x) for x in _TPL.search(name).groups())
    pieces, waves = 3 * (band + 1) * 3 * ((th + 4) // 4), th
    return (pieces + waves - 1) // waves


def device_asm():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "llicti.s")
        subprocess.check_call([hipcc] + FLAGS + ["-DCNN_STAGE_FAST=0", "-S", "--cuda-device-only", "-o", out, SRC], stderr=subprocess.DEVNULL)
        return cnn_wait_audit.kernels(out)


def _op(line):
    m = cnn_wait_audit._INSTR.match(line)
    return m.group(1) if m else None


def blocks(lines):
    """basic blocks of the kernel: [{ops: [...], succ: {block index}, in_loop: inside the tile loop}] (cold blocks of the loop's code lie behind its end)"""
    lo, hi = cnn_wait_audit.tile_loop(lines)
    body = lines
    label_at, leaders = {}, {0}
    for i, l in enumerate(body):
        m = cnn_wait_audit._LABEL.match(l)
        if m:
            label_at[m.group(1)] = i
            leaders.add(i)
        elif cnn_wait_audit._BRANCH.match(l):
            leaders.add(i + 1)
    starts = sorted(x for x in leaders if x < len(body))
    index = {s: n for n, s in enumerate(starts)}
    out = []
    for n, s in enumerate(starts):
        e = starts[n + 1] if n + 1 < len(starts) else len(body)
        ops = [l for l in body[s:e] if _op(l)]
        succ, fall = set(), True
        if ops:
            m = cnn_wait_audit._BRANCH.match(ops[-1])
            if m:
                if m.group(1) in label_at:
                    succ.add(index[label_at[m.group(1)]])
                fall = not ops[-1].strip().startswith("s_branch")
        if fall and n + 1 < len(starts):
            succ.add(n + 1)
        out.append({"ops": ops, "succ": succ, "in_loop": lo <= s <= hi})
    return out


def _kind(op):
    return "dma" if op.startswith("global_load_lds") else "vector" if op.startswith("v_") else "scalar"


def sites(lines):
    """one entry per staging site of the tile loop: {pieces, straight, loop: {vector, scalar, dma, total} | None}"""
    bl = blocks(lines)
    staging = [bool(b["ops"]) and not any(_NOT_STAGING.match(_op(l)) for l in b["ops"]) for b in bl]
    adj = {n: set() for n, ok in enumerate(staging) if ok}
    for n in adj:
        for s in bl[n]["succ"]:
            if s in adj:
                adj[n].add(s)
                adj[s].add(n)
    seen, out = set(), []
    for n in sorted(adj):
        if n in seen:
            continue
        comp, todo = set(), [n]
        while todo:
            x = todo.pop()
            if x not in comp:
                comp.add(x)
                todo.extend(adj[x] - comp)
        seen |= comp
        dma = [x for x in comp if any(_kind(_op(l)) == "dma" for l in bl[x]["ops"])]
        if not dma or not any(bl[x]["in_loop"] for x in comp):         # (the first tile's staging, in front of the loop, is not a site of it)
            continue
        # a rolled loop: a run of blocks x .. y of the site with a branch from y back to x and ONE request inside
        loop = set()
        for y in comp:
            for x in bl[y]["succ"]:
                if x <= y and x in comp and all(z in comp for z in range(x, y + 1)):
                    run, inside, todo = set(range(x, y + 1)), set(), [x]
                    while todo:                                  # (a loop only if y is reached from x inside the run: cold blocks branch back too)
                        z = todo.pop()
                        if z not in inside:
                            inside.add(z)
                            todo.extend(bl[z]["succ"] & run - inside)
                    if y in inside and sum(_kind(_op(l)) == "dma" for z in run for l in bl[z]["ops"]) == 1 and len(run) > len(loop):
                        loop = run
        count = lambda bs: {k: sum(_kind(_op(l)) == k for z in bs for l in bl[z]["ops"]) for k in ("vector", "scalar", "dma")}
        lp = count(loop) if loop else None
        if lp:
            lp["total"] = sum(lp.values())
        st = count(comp - loop)
        out.append({"pieces": st["dma"], "straight": sum(st.values()), "straight_vector": st["vector"], "loop": lp})
    return out


def parse(kernels, select=()):
    """[{kernel, wave_pieces, sites, pieces, straight, loop, per_piece}]: the site with the largest per_piece of every instantiation"""
    res = []
    for name, lines in kernels.items():
        if select and not any(s in name for s in select):
            continue
        n, best = wave_pieces(name), None
        ss = sites(lines)
        for s in ss:
            if s["pieces"]:
                s["per_piece"] = round(s["straight"] / s["pieces"], 1)
            else:
                s["per_piece"] = round(s["loop"]["total"] + s["straight"] / n, 1)
            if best is None or s["per_piece"] > best["per_piece"]:
                best = s
        res.append(dict(best, kernel=name, wave_pieces=n, sites=len(ss)))
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    opt = {}
    for flag in ("--asm", "--json"):
        if flag in args:
            i = args.index(flag)
            opt[flag] = args[i + 1]
            del args[i:i + 2]
    table = parse(cnn_wait_audit.kernels(opt["--asm"]) if "--asm" in opt else device_asm(), args)
    for k in table:
        lp = k["loop"]
        print(f"{k['kernel'][:52]:52s} sites {k['sites']}  pieces {k['pieces']:2d}/{k['wave_pieces']:2d}  straight {k['straight']:4d} ({k['straight_vector']:3d} vector)  "
              + (f"loop {lp['total']:3d} ({lp['vector']} vector, {lp['scalar']} scalar)  " if lp else "no loop  ") + f"per piece {k['per_piece']}")
    if "--json" in opt:
        json.dump(table, open(opt["--json"], "w"), indent=1)
