"""Do two builds of the library hold the same device code?

`python tools/device_code_diff.py A.s B.s` compares two device assemblies of llicti_hip.hip -- hipcc with the flags of tools/kernel_resources.py
plus `-S --cuda-device-only`, which needs no GPU -- per kernel symbol, not as files: the order of template instantiations follows the host code
and moves with it.  A function's body runs from its `NAME:` label to its `.Lfunc_end`; `;` comments are dropped (the basic-block comments carry
the function's index in the file) and local `.L...` labels are renumbered by first appearance inside the function.  Each kernel's entry in the
`amdhsa.kernels` metadata is compared verbatim.  Prints the symbols that differ and one result line; exit status 1 if anything differs.

A change that touches only host code must come out as: the same symbols, 0 differing bodies, 0 differing metadata blocks.
"""
from __future__ import annotations

import re
import sys


def function_bodies(txt):
    """{symbol: normalised body} of every function of a device assembly."""
    bodies = {}
    lines = txt.split("\n")
    i = 0
    while i < len(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", lines[i])
        if not m or m.group(1).startswith(".L"):
            i += 1
            continue
        name, body, j = m.group(1), [], i + 1
        while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
            body.append(lines[j])
            j += 1
        if j == len(lines):          # a label that opens no function (data)
            i += 1
            continue
        labels = {}

        def renumber(mm):
            return labels.setdefault(mm.group(0), ".L%d" % len(labels))

        norm = []
        for ln in body:
            ln = ln.split(";", 1)[0].rstrip()
            if ln.strip():
                norm.append(re.sub(r"\.L[\w$.]+", renumber, ln))
        bodies[name] = "\n".join(norm)
        i = j + 1
    return bodies


def kernel_metadata(txt):
    """{symbol: its entry of the amdhsa.kernels list, verbatim}"""
    md = txt[txt.index("amdhsa.kernels:"):]
    md = md[:md.index("amdhsa.target")] if "amdhsa.target" in md else md
    out = {}
    for blk in re.split(r"\n  - (?=\.)", md)[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if m:
            out[m.group(1)] = blk.rstrip()
    return out


def compare(a_txt, b_txt):
    """-> (kernels of A, kernels of B, symbols whose bodies differ, kernels whose metadata differs)"""
    fa, fb = function_bodies(a_txt), function_bodies(b_txt)
    ma, mb = kernel_metadata(a_txt), kernel_metadata(b_txt)
    bodies = sorted(n for n in set(fa) | set(fb) if fa.get(n) != fb.get(n))
    meta = sorted(n for n in set(ma) | set(mb) if ma.get(n) != mb.get(n))
    return sorted(ma), sorted(mb), bodies, meta


def main(argv):
    if len(argv) != 2:
        print(__doc__)
        return 2
    with open(argv[0]) as f:
        a_txt = f.read()
    with open(argv[1]) as f:
        b_txt = f.read()
    ka, kb, bodies, meta = compare(a_txt, b_txt)
    for n in sorted(set(ka) ^ set(kb)):
        print("kernel only in %s: %s" % ("A" if n in ka else "B", n))
    for n in bodies:
        print("body differs: %s" % n)
    for n in meta:
        print("metadata differs: %s" % n)
    same_names = ka == kb
    print("device code: %d kernels in A, %d in B, %s symbol names; %d differing bodies, %d differing metadata blocks"
          % (len(ka), len(kb), "the same" if same_names else "DIFFERENT", len(bodies), len(meta)))
    return 0 if same_names and not bodies and not meta else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
