#!/usr/bin/env python3
"""Which vector instructions does the band CNN's tile loop issue beside its MFMAs?  Inventory from the device assembly (no GPU needed).

    python tools/cnn_valu_audit.py [--asm llicti.s] [--json out.json] [kernel-name substring ...]

Without --asm the tool compiles llicti_hip.hip itself with the product flags (tools/kernel_resources.py FLAGS).

A vector instruction occupies the SIMD's vector issue port for 4 cycles, the port the MFMAs issue through too (rounds 9
and 10): whatever the tile loop computes there that is no matrix work -- and address arithmetic above all -- is paid for.  Per band_params*_kernel
instantiation the tile loop (tools/cnn_wait_audit.py: the outermost loop around the s_barrier) is cut into basic blocks (tools/cnn_border_isa.py);
the MFMA BLOCKS are the ones that hold a v_mfma.  The table lists
    mfma            MFMAs of the tile loop
    valu            non-MFMA vector instructions (v_*) of the MFMA blocks, and `valu_by_op`, the same by mnemonic
    lit_add_ds      v_add_u32 vN, <immediate>, vM of the MFMA blocks whose result is the address of a ds_read* before vN is written again:
                    an LDS address re-derived in front of a read instead of base register + offset field;  `lit_add_ds_hi` those with an
                    immediate >= 0x10000 (beyond a DS instruction's 16-bit offset), counted over the WHOLE kernel; add and read in ONE block
                    (see lit_adds_to_ds)
    addr_mul        v_mul_lo_u32 / v_mul_hi_u32 / v_mad_u64_u32 / v_mad_i64_i32 of the MFMA blocks (the epilogue's address products)
    epi_mul, epi_add64   the same multiplies, and the 64-bit vector adds (v_lshl_add_u64, v_add_co_u32 / v_addc_co_u32 pairs count once),
                    behind the tile's last MFMA up to the end of the loop: the params stores' address arithmetic
    stores          global_store_* instructions of the loop
parse() is what tests/test_cnn_valu_budget_cpu.py asserts through."""
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cnn_border_isa                                    # noqa: E402
import cnn_wait_audit                                    # noqa: E402
from kernel_resources import FLAGS, SRC                  # noqa: E402

_LIT_ADD = re.compile(r"^\s+v_add_u32(?:_e32|_e64)?\s+v(\d+),\s*(0x[0-9a-fA-F]+|-?\d+),\s*v\d+\s*$")
_DEST = re.compile(r"^\s+[a-z_0-9]+\s+(?:v(\d+)|v\[(\d+):(\d+)\])\b")
_DS_READ = re.compile(r"^\s+ds_read\w*\s+(?:v\d+|v\[\d+:\d+\]),\s*v(\d+)\b")
_MULS = ("v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32", "v_mad_i64_i32")
_ADD64 = ("v_lshl_add_u64", "v_addc_co_u32")


def device_asm():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "llicti.s")
        subprocess.check_call([hipcc] + FLAGS + ["-S", "--cuda-device-only", "-o", out, SRC], stderr=subprocess.DEVNULL)
        return cnn_wait_audit.kernels(out)


def _op(line):
    return cnn_border_isa._op(line).replace("_e32", "").replace("_e64", "")


def lit_adds_to_ds(ops):
    """immediates of the v_add_u32 vN, <immediate>, vM in `ops` (one basic block) whose vN is a ds_read's address before it is overwritten.
    An add is followed to its read inside its own block only: one whose result is first read in a later block is NOT counted -- neither here nor
    in the whole-kernel count of adds >= 0x10000.  (Following it further cannot tell a per-tile add from a base the compiler made once in
    front of the loop, which costs nothing per tile: the 8- and 4-row forms of band 2 keep such bases.)  Inside the MFMA blocks the total
    `valu` count sees every add regardless of where its result is read."""
    out, pending = [], {}
    for l in ops:
        m = _DS_READ.match(l)
        if m and int(m.group(1)) in pending:
            out.append(pending.pop(int(m.group(1))))
        d = _DEST.match(l)
        if d and not l.lstrip().startswith("ds_write"):
            lo = int(d.group(1) if d.group(1) is not None else d.group(2))
            hi = int(d.group(3)) if d.group(3) is not None else lo
            for r in range(lo, hi + 1):
                pending.pop(r, None)
        a = _LIT_ADD.match(l)
        if a:
            pending[int(a.group(1))] = int(a.group(2), 0)
    return out


def audit(lines):
    bl = cnn_border_isa.blocks(lines)
    loop = [b for b in bl if b["in_loop"]]
    mf = [b for b in loop if any(_op(l).startswith("v_mfma") for l in b["ops"])]
    by_op = collections.Counter(_op(l) for b in mf for l in b["ops"] if _op(l).startswith("v_") and not _op(l).startswith("v_mfma"))
    lit = [c for b in mf for c in lit_adds_to_ds(b["ops"])]
    lit_all = [c for b in bl for c in lit_adds_to_ds(b["ops"])]
    # the epilogue: everything of the loop behind its last MFMA
    flat = [l for b in loop for l in b["ops"]]
    last = max(i for i, l in enumerate(flat) if _op(l).startswith("v_mfma"))
    epi = [_op(l) for l in flat[last + 1:]]
    return {"mfma": sum(_op(l).startswith("v_mfma") for l in flat), "mfma_blocks": len(mf),
            "valu": sum(by_op.values()), "valu_by_op": dict(sorted(by_op.items())),
            "lit_add_ds": len(lit), "lit_add_ds_by_block": [len(lit_adds_to_ds(b["ops"])) for b in mf],
            "lit_add_ds_hi": sum(c >= 0x10000 for c in lit_all),
            "addr_mul": sum(by_op[m] for m in _MULS),
            "epi_mul": sum(o in _MULS for o in epi), "epi_add64": sum(o in _ADD64 for o in epi),
            "stores": sum(_op(l).startswith("global_store") for l in flat)}


def parse(kernels, select=()):
    """[{kernel, config, band, rows, mixed, mfma, valu, valu_by_op, lit_add_ds, ...}] for every band_params*_kernel instantiation"""
    res = []
    for name, lines in kernels.items():
        if select and not any(s in name for s in select):
            continue
        band, th, ragged = (int(x) for x in cnn_border_isa._TPL.search(name).groups())
        res.append(dict({"kernel": name, "config": "B" if "h60" in name else "A", "band": band, "rows": th, "mixed": bool(ragged)}, **audit(lines)))
    return sorted(res, key=lambda k: (k["config"], k["mixed"], -k["rows"], k["band"]))


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
        top = ", ".join(f"{o[2:]} {n}" for o, n in sorted(k["valu_by_op"].items(), key=lambda x: -x[1])[:6])
        print(f"{k['config']} band {k['band']} rows {k['rows']:2d} {'mixed' if k['mixed'] else 'equal'}: mfma {k['mfma']:4d}  valu {k['valu']:3d}  "
              f"lit-add->ds {k['lit_add_ds']:3d} {k['lit_add_ds_by_block']} (>=64K: {k['lit_add_ds_hi']})  addr-mul {k['addr_mul']}  "
              f"epilogue mul {k['epi_mul']} add64 {k['epi_add64']}  stores {k['stores']}  | {top}")
    if "--json" in opt:
        json.dump(table, open(opt["--json"], "w"), indent=1)
