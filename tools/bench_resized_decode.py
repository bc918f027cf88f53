#!/usr/bin/env python
"""Resized crops: does one decode_tensor_resized call beat today's way to the same [B, 3, 224, 224] float16 training tensor?

  python tools/bench_resized_decode.py [--reps 20] [--warmup 3] [--size 224] [--out profiles/resized_decode/bench.json]

Natural-like images (llicti_amd/synth.py "smooth"), seed-1337 weights.  Every image gets a box drawn as torchvision's RandomResizedCrop draws it
(scale 0.08 .. 1, log-uniform ratio 3/4 .. 4/3, ten tries, then the centre fallback; restated here, seeded, the same for both legs) and a random
horizontal flip; ImageNet mean / std.
  workload "uniform"  24 x 768x512 in container xrans15.  Most boxes are smaller than 448 px, so resized_crop_plan keeps reduce = 0 and both legs
                      decode every level: no headline gain is expected, the legs differ in the passes behind the decode.
  workload "uhd"      8 x 3840x2160 in container "auto".  resized_crop_plan picks reduce from the boxes: the finest level or levels are never
                      decoded by leg B (a DECIMATION: leg B's pixels are then not leg A's, see the recorded difference).  reduce is one value
                      per call and the filter takes a scale of at most 4, while the boxes of one UHD batch differ by more than that: where the
                      common reduce would leave a box above 4, leg B groups the images by the reduce each affords alone -- one call per group.
  leg A  today's way: decode_v at full size, then per image slice, F.interpolate(bilinear, antialias=True), / 255, normalise, flip; torch.stack, .half()
  leg B  ONE HipCodec.decode_tensor_resized call (llicti_decode_images_tensor_resized) at resized_crop_plan's reduce (uhd: one per reduce group)
One round = A then B between device events on the compute stream, `--reps` rounds (at least 5) after `--warmup` untimed ones in ONE process, so
clock and temperature drift hit both alike; medians, min .. max and p10 .. p90 are reported.  Where reduce = 0 the two legs compute the same
filter in different fp32 orders: their largest difference is recorded and must stay within two float16 steps of the value range, or the run
fails after the file is written.  No speed target is set.

The driver itself never touches the GPU: every workload is a child process under its own `timeout`, and the first one that fails ends the run.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def stats(v):
    s = sorted(v)
    n = len(s)

    def pct(p):
        return s[min(n - 1, max(0, int(round(p * (n - 1)))))]
    return {"median_ms": round(statistics.median(s), 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4), "p10_ms": round(pct(0.1), 4),
            "p90_ms": round(pct(0.9), 4), "reps": n}


def random_resized_box(rng, H, W, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
    """torchvision.transforms.RandomResizedCrop.get_params, restated: -> (y0, x0, h, w)"""
    area = H * W
    for _ in range(10):
        target = area * rng.uniform(*scale)
        ar = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
        w, h = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
        if 0 < w <= W and 0 < h <= H:
            return int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w
    in_ratio = W / H
    if in_ratio < ratio[0]:
        w, h = W, int(round(W / ratio[0]))
    elif in_ratio > ratio[1]:
        h, w = H, int(round(H * ratio[1]))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def measure(name, reps, warmup, size):
    """The child's work: one workload, both legs in one process; -> dict."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    from llicti_amd.codec import HipCodec, auto_modes, mode_of_name, name_of_mode, resized_crop_plan
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    from llicti_amd.synth import make_image
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1337)
    sd = LLICTI(default_config()).state_dict()
    sizes = [(512, 768)] * 24 if name == "uniform" else [(2160, 3840)] * 8
    distinct = 4 if name == "uniform" else 2              # (the generator is slow)
    B = len(sizes)
    Hs, Ws = [h for h, _ in sizes], [w for _, w in sizes]
    rng = np.random.default_rng(7)
    full = [random_resized_box(rng, h, w) for h, w in sizes]
    flip = [int(v) for v in rng.integers(0, 2, B)]
    # ONE reduce per call.  The batch's common value (resized_crop_plan) serves unless a box then shrinks by more than 4, the filter's limit --
    # boxes of one UHD batch differ by more than that -- in which case the images are grouped by the reduce each affords alone, one call per
    # group (the batch is put in group order up front, so every group reads and writes one contiguous slice).
    reduce, boxes = resized_crop_plan(sizes, full, (size, size))
    groups = [(reduce, 0, B)]
    if any(h > 4 * size or w > 4 * size for _, _, h, w in boxes):
        own = [resized_crop_plan([sizes[b]], [full[b]], (size, size))[0] for b in range(B)]
        order = sorted(range(B), key=lambda b: own[b])
        full, flip, own = [full[b] for b in order], [flip[b] for b in order], [own[b] for b in order]
        groups, boxes = [], []
        for r in sorted(set(own)):
            lo, hi = own.index(r), B - own[::-1].index(r)
            groups.append((r, lo, hi))
            boxes += resized_crop_plan(sizes[lo:hi], full[lo:hi], (size, size))[1]
    made = [make_image("smooth", sizes[0][0], sizes[0][1], 100 + i) for i in range(distinct)]
    imgs = [made[i % distinct] for i in range(B)]
    c = HipCodec(dev)
    c.load_state_dict(sd)
    offs, total = c.flat_offsets(Hs, Ws)
    if name == "uniform":
        enc_mode = mode_of_name("xrans15")
    else:
        m = auto_modes(sizes)
        enc_mode = m[0] if all(v == m[0] for v in m) else m
    cont, seg = c.encode_v(torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(dev), Hs, Ws, enc_mode)
    c.check()
    dm = c.container_modes(cont)
    assert all(v == dm[0] for v in dm)                   # (equal sizes: one mode)
    dec_mode = dm[0]
    mean_t = torch.tensor(MEAN, dtype=torch.float32, device=dev)[:, None, None]
    std_t = torch.tensor(STD, dtype=torch.float32, device=dev)[:, None, None]
    t255 = torch.tensor(255.0, dtype=torch.float32, device=dev)
    flat_buf = torch.empty((total,), dtype=torch.uint8, device=dev)
    out_b = torch.empty((B, 3, size, size), dtype=torch.float16, device=dev)

    def leg_a():
        flat = c.decode_v(cont, seg, Hs, Ws, dec_mode, out=flat_buf)
        outs = []
        for b in range(B):
            y0, x0, h, w = full[b]
            win = flat[int(offs[b]):int(offs[b]) + 3 * Hs[b] * Ws[b]].view(3, Hs[b], Ws[b])[:, y0:y0 + h, x0:x0 + w]
            x = F.interpolate(win.float()[None], size=(size, size), mode="bilinear", align_corners=False, antialias=True)[0]
            x = (x / t255 - mean_t) / std_t
            outs.append(torch.flip(x, dims=[-1]) if flip[b] else x)
        return torch.stack(outs).to(torch.float16)

    def leg_b(bx=None):
        bx = boxes if bx is None else bx
        for r, lo, hi in groups:
            c.decode_tensor_resized(cont[lo:hi], seg[lo:hi], Hs[lo:hi], Ws[lo:hi], dec_mode, (size, size), bx[lo:hi], dtype=torch.float16, flip=flip[lo:hi],
                                    mean=MEAN, std=STD, antialias=True, reduce=r, out=out_b[lo:hi])
        return out_b
    c.poison_workspace()
    got_a = leg_a()
    c.poison_workspace()
    got_b = leg_b().clone()
    c.check()
    diff = float((got_a.float() - got_b.float()).abs().max())

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    cols = {"a": [], "b": []}
    for k in range(warmup + reps):
        t = {"a": timed(leg_a), "b": timed(leg_b)}
        if k >= warmup:
            for key, v in t.items():
                cols[key].append(v)
    c.check()
    counters = ("plan_builds", "plan_hits", "device_syncs", "device_allocs")
    before = {k: c.counter(k) for k in counters}
    for k in range(4):                                   # new boxes every call, in the same groups: plan hits and nothing else
        bx = []
        for r, lo, hi in groups:                         # (mapped onto the group's grid, cut to the filter's scale of 4)
            for b in range(lo, hi):
                y0, x0, h, w = random_resized_box(rng, *sizes[b])
                bx.append((y0 >> r, x0 >> r, max(1, min(h >> r, 4 * size)), max(1, min(w >> r, 4 * size))))
        leg_b(bx)
    after = {k: c.counter(k) for k in counters}
    c.set_profiling(True)
    prof = {}
    for key, fn in (("a_decode_v", lambda: c.decode_v(cont, seg, Hs, Ws, dec_mode, out=flat_buf)), ("b_decode_tensor_resized", leg_b)):
        fn()
        cat, per = c.last_timing_detail()
        prof[key] = {"band_cnn_launches": len(per), "kernel_group_ms": {k: round(v, 4) for k, v in cat.items()}}
    c.set_profiling(False)
    c.check()
    c.close()
    a, b = stats(cols["a"]), stats(cols["b"])
    modes = enc_mode if isinstance(enc_mode, list) else [enc_mode]
    return {"device": torch.cuda.get_device_name(dev), "images": B, "sizes": sorted({f"{w}x{h}" for h, w in sizes}),
            "megapixels": round(sum(h * w for h, w in sizes) / 1e6, 3), "container": sorted({name_of_mode(m) for m in modes}),
            "output": f"[{B}, 3, {size}, {size}] float16, random resized crop + flip per image, ImageNet mean / std",
            "boxes_full_resolution_yxhw": [list(v) for v in full], "reduce": min(r for r, _, _ in groups),
            "calls_of_leg_b": [{"reduce": r, "images": hi - lo} for r, lo, hi in groups],
            "ms": {"a": a, "b": b, "b_minus_a_ms": round(b["median_ms"] - a["median_ms"], 4), "a_over_b": round(a["median_ms"] / b["median_ms"], 3)},
            "max_abs_difference_a_b": diff, "difference_note": "reduce = 0: the same filter in two fp32 orders, rounded to float16; reduce >= 1: leg B resamples a "
            "decimated image, leg A low-passes the full one -- they are different pictures",
            "four_calls_with_new_boxes": {k: after[k] - before[k] for k in counters}, "profiled_calls": prof}


def run_step(what, cmd, cwd, seconds):
    """One GPU step: a child of its own under `timeout`; -> its last JSON line, or raises (the run ends there)."""
    print(f"[{what}] timeout {seconds} s: {' '.join(cmd)}", flush=True)
    p = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, cwd=cwd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"[{what}] exit status {p.returncode}: nothing more is started")
    for line in reversed(p.stdout.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise SystemExit(f"[{what}] printed no JSON line")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=224, help="side of the square output")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resized_decode", "bench.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.reps < 5:
        ap.error("--reps: at least 5 timed repetitions")
    if a.child:
        print(json.dumps(measure(a.child, a.reps, a.warmup, a.size)))
        return 0
    out = {"tool": "tools/bench_resized_decode.py", "reps": a.reps, "warmup": a.warmup,
           "metric": "ms per call sequence between device events; A = full-size decode + torch passes per image, B = one call of this library",
           "workloads": {}}
    for name in ("uniform", "uhd"):
        out["workloads"][name] = run_step(name, [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps),
                                                 "--warmup", str(a.warmup), "--size", str(a.size)], ROOT, 420)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    bad = []
    for name, w in out["workloads"].items():
        m = w["ms"]
        print("%-8s reduce %d   A %.3f ms (min %.3f, max %.3f)   B %.3f ms (min %.3f, max %.3f)   A / B %.2f   max |A - B| %.4g" % (
            name, w["reduce"], m["a"]["median_ms"], m["a"]["min_ms"], m["a"]["max_ms"], m["b"]["median_ms"], m["b"]["min_ms"], m["b"]["max_ms"],
            m["a_over_b"], w["max_abs_difference_a_b"]))
        if w["reduce"] == 0 and w["max_abs_difference_a_b"] > 2 * 2.0 ** -9:      # two float16 steps at |x| in 2 .. 4, the top of the normalised range
            bad.append(name)
    print("wrote", a.out)
    if bad:
        raise SystemExit(f"leg B differs from leg A by more than two float16 steps on {bad} at reduce 0")
    return 0


if __name__ == "__main__":
    sys.exit(main())
