#!/usr/bin/env python3
"""Where does the band CNN wait for vector memory?  Audit of the compiled kernels' tile loops.

    hipcc <llicti_amd._lib.HIPCC_FLAGS without -shared> -S --cuda-device-only -o llicti.s llicti_amd/csrc/llicti_hip.hip
    python tools/cnn_wait_audit.py llicti.s [--json out.json] [kernel-name substring ...]

For every band_params*_kernel instantiation (or the ones whose mangled name contains one of the substrings, e.g. "ILi2ELi16ELb0E")
the table lists each s_waitcnt that has a vmcnt field INSIDE THE TILE LOOP (the outermost loop that holds the s_barrier): its count, the
number of LDS-DMA requests (global_load_lds_*) and of global stores in program order since the previous such wait, and the next LDS
instruction or barrier behind it.  The input staging is LDS-DMA tracked by vmcnt: a wait the compiler puts in front of a ds_read inside
the loop would stall a wavefront for a memory round trip per tile (the kernel's only intended wait is the explicit vmcnt(0) in front of
the tile's barrier).  parse() is what tests/test_cnn_isa_cpu.py asserts through."""
import json
import re
import sys

_KERNEL = re.compile(r"^(_Z\d+band_params\w*_kernel\w+):")
_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")
_VMCNT = re.compile(r"^\s+s_waitcnt\b.*\bvmcnt\((\d+)\)")
_INSTR = re.compile(r"^\s+([a-z_0-9]+)\b")


def kernels(path):
    """{mangled name: [instruction / label lines]} of every band_params*_kernel in the assembly file"""
    out, cur = {}, None
    for line in open(path):
        m = _KERNEL.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        line = line.split(";")[0].rstrip()
        if not line:
            continue
        cur.append(line)
        if line.strip() == "s_endpgm":
            cur = None
    return out


def tile_loop(lines):
    """(first, last) line index of the outermost loop around the s_barrier: the widest backward branch that spans it"""
    labels = {m.group(1): i for i, m in ((i, _LABEL.match(l)) for i, l in enumerate(lines)) if m}
    barriers = [i for i, l in enumerate(lines) if l.strip() == "s_barrier"]
    assert barriers, "no s_barrier in the kernel"
    b, best = barriers[0], None
    for i, l in enumerate(lines):
        m = _BRANCH.match(l)
        if m and m.group(1) in labels and labels[m.group(1)] <= b <= i:
            if best is None or (i - labels[m.group(1)]) > (best[1] - best[0]):
                best = (labels[m.group(1)], i)
    assert best is not None, "the s_barrier is in no loop"
    return best


def parse(path, select=()):
    """[{kernel, loop_lines, barriers, dma_in_loop, waits: [{line, vmcnt, dma_since, stores_since, next}]}]"""
    res = []
    for name, lines in kernels(path).items():
        if select and not any(s in name for s in select):
            continue
        lo, hi = tile_loop(lines)
        waits, dma, st = [], 0, 0
        for i in range(lo, hi + 1):
            m = _INSTR.match(lines[i])
            if not m:
                continue
            op = m.group(1)
            if op.startswith("global_load_lds") or (op.startswith("buffer_load") and " lds" in lines[i]):
                dma += 1
            elif op.startswith("global_store") or op.startswith("buffer_store") or op.startswith("flat_store"):
                st += 1
            w = _VMCNT.match(lines[i])
            if w:
                nxt = next((mm.group(1) for mm in (_INSTR.match(l) for l in lines[i + 1:hi + 1])
                            if mm and (mm.group(1).startswith("ds_") or mm.group(1) == "s_barrier")), None)
                waits.append({"line": i - lo, "vmcnt": int(w.group(1)), "dma_since": dma, "stores_since": st, "next": nxt})
                dma, st = 0, 0
        res.append({"kernel": name, "loop_lines": hi - lo + 1,
                    "barriers": sum(1 for l in lines[lo:hi + 1] if l.strip() == "s_barrier"),
                    "dma_in_loop": sum(1 for l in lines[lo:hi + 1] if "global_load_lds" in l), "waits": waits})
    return res


def merged(waits):
    """back-to-back waits with nothing issued between them (the explicit drain and the fence's own) count as one"""
    out = []
    for w in waits:
        if out and w["dma_since"] == 0 and w["stores_since"] == 0 and w["line"] - out[-1]["line"] <= 3:
            continue
        out.append(w)
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    jout = None
    if "--json" in args:
        i = args.index("--json")
        jout = args[i + 1]
        del args[i:i + 2]
    table = parse(args[0], args[1:])
    for k in table:
        print(f"{k['kernel']}: tile loop {k['loop_lines']} lines, {k['barriers']} barrier, {k['dma_in_loop']} LDS-DMA instructions")
        for w in k["waits"]:
            print(f"    +{w['line']:<6} vmcnt({w['vmcnt']})  LDS-DMA since previous {w['dma_since']:3}  stores {w['stores_since']:2}  next: {w['next']}")
    if jout:
        json.dump(table, open(jout, "w"), indent=1)
