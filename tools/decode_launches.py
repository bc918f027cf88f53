#!/usr/bin/env python3
"""Every whole-batch decode entry point once, for a kernel trace that two builds of the library can be compared on:

    rocprofv3 --kernel-trace --output-format csv -d OUT -o t -- python3 tools/decode_launches.py      (LLICTI_HIP_SO picks the build)
    python3 tools/decode_launches.py --list OUT/.../t_kernel_trace.csv launches.json
    python3 tools/decode_launches.py --compare a.json b.json verdict.json [launches.json]

The run: a uniform batch (two 64x96 images) and a mixed one (48x80, 96x64, 33x127) as rANS containers, the uniform one in the reference format
too; the thirteen calls (llicti_decode_images, _v, _vm, _reduced, _px, _tensor, _tensor_resized, _tensor_views and the five _rv) at reduce 0 and
1 and, for the rANS containers, per-image [0, 1] / [1, 0, 2]; an all-equal list stands for the _rv calls on the reference format.  It prints a
digest of every byte the calls wrote, so that the two builds' outputs can be held against each other as well.
--list: the trace's dispatches in the order the host made them -> [[kernel, grid x, y, z, workgroup x], ...].
--compare: the two lists identical, or the first place they differ; with their digests.  launches.json: list a in short form -- the distinct
launches, and per decode call (a run from one zero_words_kernel to the next) the indices of its launches in host order."""
import csv
import hashlib
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run():
    import numpy as np
    import torch
    from llicti_amd.codec import HipCodec, MODE_AC, MODE_RANS
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI

    torch.manual_seed(1337)
    codec = HipCodec(torch.device("cuda", 0))
    codec.load_state_dict(LLICTI(default_config()).state_dict())
    rng = np.random.default_rng(7)
    digest = hashlib.sha256()
    n_calls = 0

    def took(*outs):
        nonlocal n_calls
        codec.check()
        n_calls += 1
        for o in outs:
            digest.update(o.contiguous().view(torch.uint8).cpu().numpy().tobytes())

    def batch(sizes, mode, per_image):
        Hs, Ws = [h for h, _ in sizes], [w for _, w in sizes]
        B = len(sizes)
        flat = torch.from_numpy(np.concatenate([rng.integers(0, 256, size=3 * h * w, dtype=np.uint8) for h, w in sizes])).to(codec.device)
        cont, seg = codec.encode_v(flat, Hs, Ws, mode)
        codec.check()
        size, mean, std = (8, 16), (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
        views = [dict(size=size, image=[B - 1, 0, B - 1], antialias=False), dict(size=(5, 7), dtype=torch.float16, antialias=False)]
        if len(set(sizes)) == 1:
            took(codec.decode(cont, seg, Hs[0], Ws[0], mode=mode))                                # llicti_decode_images
        took(codec.decode_v(cont, seg, Hs, Ws, mode))                                             # llicti_decode_images_v
        for r in [0, 1, [1] * B] + ([per_image] if per_image else []):                            # scalar calls, then the _rv ones
            took(codec.decode_reduced(cont, seg, Hs, Ws, mode, r))
            took(codec.decode_px(cont, seg, Hs, Ws, mode, fmt="bgra", reduce=r))
            took(codec.decode_tensor(cont, seg, Hs, Ws, mode, size, dtype=torch.float16, flip=[1] + [0] * (B - 1), mean=mean, std=std, reduce=r))
            took(codec.decode_tensor_resized(cont, seg, Hs, Ws, mode, size, None, antialias=False, reduce=r))
            took(*codec.decode_tensor_views(cont, seg, Hs, Ws, mode, views, mean=mean, std=std, reduce=r))
        if per_image:                                                                             # llicti_decode_images_vm: stream counts that differ
            modes = [MODE_RANS(3 + b, wide=2) for b in range(B)]
            cont, seg = codec.encode_v(flat, Hs, Ws, modes)
            took(codec.decode_v(cont, seg, Hs, Ws, modes))

    uniform, mixed = [(64, 96)] * 2, [(48, 80), (96, 64), (33, 127)]
    batch(uniform, MODE_RANS(4, wide=2), [0, 1])
    batch(mixed, MODE_RANS(4, wide=2), [1, 0, 2])
    batch(uniform, MODE_AC, None)
    torch.cuda.synchronize()
    print(f"decode_launches: {n_calls} calls, outputs sha256 {digest.hexdigest()}")


def launches(trace_csv):
    with open(trace_csv, newline="") as f:
        rows = list(csv.DictReader(f))
    order = "Dispatch_Id" if rows and "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[order]))
    return [[re.sub(r"^void ", "", re.sub(r"\(.*", "", r["Kernel_Name"]))] + [int(r.get(k, 0) or 0) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X")]
            for r in rows]


def main(argv):
    if argv[:1] == ["--list"]:
        ls = launches(argv[1])
        with open(argv[2], "w") as f:
            json.dump(ls, f, separators=(",", ":"))
        print(f"{len(ls)} dispatches -> {argv[2]}")
    elif argv[:1] == ["--compare"]:
        a, b = (json.load(open(p)) for p in argv[1:3])
        diff = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
        sha = [hashlib.sha256(json.dumps(x, separators=(",", ":")).encode()).hexdigest() for x in (a, b)]
        verdict = {"a": os.path.basename(argv[1]), "b": os.path.basename(argv[2]), "dispatches": [len(a), len(b)], "sha256": sha, "identical": diff is None,
                   "first_difference": None if diff is None else {"index": diff, "a": a[diff:diff + 1], "b": b[diff:diff + 1]}}
        with open(argv[3], "w") as f:
            json.dump(verdict, f, indent=1)
        print(json.dumps(verdict))
        if len(argv) > 4:
            shapes = sorted(set(map(tuple, a)))
            calls = []
            for x in a:
                if x[0] == "zero_words_kernel" or not calls:
                    calls.append([])
                calls[-1].append(str(shapes.index(tuple(x))))
            with open(argv[4], "w") as f:
                f.write('{"launch": ["kernel", "grid x", "grid y", "grid z", "workgroup x"],\n "launches": [\n  ' + ",\n  ".join(json.dumps(list(x)) for x in shapes) +
                        '],\n "calls": [\n  ' + ",\n  ".join(json.dumps(" ".join(c)) for c in calls) + "]}\n")
        return 0 if diff is None else 1
    else:
        run()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
