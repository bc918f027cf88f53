#!/usr/bin/env python
"""Tensor options: what do the channels-last layout and the padded windows of the decode's last kernel save over the torch passes they replace?

  python tools/bench_tensor_layout.py [--reps 20] [--warmup 3] [--out profiles/tensor_layout/bench.json]

Container "auto", seed-1337 weights, ImageNet mean / std, float16 outputs, images from llicti_amd/synth.py "smooth".
  workload "nhwc_resized"  24 images of 768x512, one random resized crop per image (tools/bench_resized_decode.py: random_resized_box, seeded) to
                           224x224, reduce as codec.resized_crop_plan picks it
     variant new   decode_tensor_resized(channels_last=True): the kernel interleaves the channels as it stores
     variant old   decode_tensor_resized, then .contiguous(memory_format=torch.channels_last): one more pass over the batch
  workload "padded_crop"   24 images of 300 .. 768 pixels per side (drawn with a fixed seed), torchvision's CenterCrop(512): most images are
                           smaller than the crop on an axis and are padded with zeros
     variant new   decode_tensor(origin=center_crop_origins(...), pad=dict(mode="constant")): one call, one [24, 3, 512, 512] tensor
     variant old   decode_v, then per image F.pad, slice, / 255, normalise; torch.stack and .half()
One round = new, old between device events on the compute stream; `--reps` rounds (at least 5) after `--warmup` untimed ones of both variants in
ONE process, alternating, so clock and temperature drift hit both alike; medians and min .. max are reported.  "nhwc_resized": the two variants
must agree bit for bit on the timed inputs, or the run fails after the file is written.  "padded_crop": whether they do is recorded with the
largest difference (the old variant's arithmetic is torch's on the device; tests/test_hip_tensor_layout.py holds the call against the CPU).
No gain is promised: the decode dominates both.

The driver itself never touches the GPU: every workload is a child process under its own `timeout`, and the first one that fails ends the run.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_resized_decode import MEAN, STD, random_resized_box, run_step, stats  # noqa: E402

WORKLOADS = ("nhwc_resized", "padded_crop")


def measure(name, reps, warmup):
    """The child's work: one workload, both variants in one process; -> dict."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    from llicti_amd.codec import HipCodec, auto_modes, center_crop_origins, name_of_mode, resized_crop_plan
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    from llicti_amd.synth import make_image
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1337)
    sd = LLICTI(default_config()).state_dict()
    B, distinct = 24, 4                                    # (the generator is slow: four distinct images, cut to size)
    rng = np.random.default_rng(11)
    if name == "nhwc_resized":
        sizes = [(512, 768)] * B
    else:
        sizes = [(int(rng.integers(300, 769)), int(rng.integers(300, 769))) for _ in range(B)]
    Hs, Ws = [h for h, _ in sizes], [w for _, w in sizes]
    made = [make_image("smooth", 768, 768, 100 + i) for i in range(distinct)]
    c = HipCodec(dev)
    c.load_state_dict(sd)
    offs, total = c.flat_offsets(Hs, Ws)
    m = auto_modes(sizes)
    enc_mode = m[0] if all(v == m[0] for v in m) else m
    flat = np.concatenate([np.ascontiguousarray(made[i % distinct][:, :h, :w]).reshape(-1) for i, (h, w) in enumerate(sizes)])
    cont, seg = c.encode_v(torch.from_numpy(flat).to(dev), Hs, Ws, enc_mode)
    c.check()
    dm = c.container_modes(cont)
    dec_mode = dm[0] if all(v == dm[0] for v in dm) else dm
    mean_t = torch.tensor(MEAN, dtype=torch.float32, device=dev)[:, None, None]
    std_t = torch.tensor(STD, dtype=torch.float32, device=dev)[:, None, None]
    t255 = torch.tensor(255.0, dtype=torch.float32, device=dev)
    extra = {}
    if name == "nhwc_resized":
        side = 224
        boxes = []
        for h, w in sizes:
            box = random_resized_box(rng, h, w)
            while box[2] > 4 * side or box[3] > 4 * side:
                box = random_resized_box(rng, h, w)
            boxes.append(box)
        reduce, mapped = resized_crop_plan(sizes, boxes, (side, side))
        flip = [int(v) for v in rng.integers(0, 2, B)]
        out_new = torch.empty((B, 3, side, side), dtype=torch.float16, device=dev, memory_format=torch.channels_last)
        out_old = torch.empty((B, 3, side, side), dtype=torch.float16, device=dev)
        kw = dict(dtype=torch.float16, flip=flip, mean=MEAN, std=STD, antialias=True, reduce=reduce)

        def var_new():
            return c.decode_tensor_resized(cont, seg, Hs, Ws, dec_mode, (side, side), mapped, out=out_new, channels_last=True, **kw)

        def var_old():
            return c.decode_tensor_resized(cont, seg, Hs, Ws, dec_mode, (side, side), mapped, out=out_old, **kw).contiguous(memory_format=torch.channels_last)
        extra = {"output": f"[{B}, 3, {side}, {side}] float16, channels_last", "reduce": reduce}
    else:
        side = 512
        origin = center_crop_origins(sizes, (side, side))
        out_new = torch.empty((B, 3, side, side), dtype=torch.float16, device=dev)
        flat_buf = torch.empty((total,), dtype=torch.uint8, device=dev)

        def var_new():
            return c.decode_tensor(cont, seg, Hs, Ws, dec_mode, (side, side), dtype=torch.float16, origin=origin, mean=MEAN, std=STD, out=out_new,
                                   pad=dict(mode="constant", fill=0))

        def var_old():
            flat_d = c.decode_v(cont, seg, Hs, Ws, dec_mode, out=flat_buf)
            outs = []
            for b, (h, w) in enumerate(sizes):
                img = flat_d[int(offs[b]):int(offs[b]) + 3 * h * w].view(3, h, w)
                y0, x0 = origin[0][b], origin[1][b]
                img = F.pad(img, (max(-x0, 0), max(x0 + side - w, 0), max(-y0, 0), max(y0 + side - h, 0)))
                y0, x0 = max(y0, 0), max(x0, 0)
                outs.append((img[:, y0:y0 + side, x0:x0 + side].float() / t255 - mean_t) / std_t)
            return torch.stack(outs).to(torch.float16)
        extra = {"output": f"[{B}, 3, {side}, {side}] float16", "images_smaller_than_the_crop_on_an_axis": sum(1 for h, w in sizes if h < side or w < side),
                 "sizes_min_max": [min(Hs), max(Hs), min(Ws), max(Ws)]}
    c.poison_workspace()
    a = var_old().clone()
    c.poison_workspace()
    b_ = var_new()
    c.check()
    equal = bool(a.shape == b_.shape and a.stride() == b_.stride() and torch.equal(a, b_))
    diff = float((a.float() - b_.float()).abs().max())

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    cols = {"new": [], "old": []}
    for k in range(warmup + reps):
        t = {"new": timed(var_new), "old": timed(var_old)}
        if k >= warmup:
            for key, v in t.items():
                cols[key].append(v)
    c.check()
    equal_after = bool(torch.equal(var_old(), var_new()))
    c.check()
    c.close()
    st = {k: stats(v) for k, v in cols.items()}
    spread = {k: round(v["max_ms"] - v["min_ms"], 4) for k, v in st.items()}
    gain = round(st["old"]["median_ms"] - st["new"]["median_ms"], 4)
    modes = enc_mode if isinstance(enc_mode, list) else [enc_mode]
    return {"device": torch.cuda.get_device_name(dev), "images": B, "container": sorted({name_of_mode(v) for v in modes}), **extra,
            "ms": {**st, "spread_ms": spread, "old_minus_new_ms": gain, "old_over_new": round(st["old"]["median_ms"] / st["new"]["median_ms"], 3)},
            "new_below_old_by_more_than_both_spreads": bool(gain > spread["new"] + spread["old"]), "new_equals_old_bit_for_bit": bool(equal and equal_after),
            "max_abs_difference_new_old": diff}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_layout", "bench.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.reps < 5:
        ap.error("--reps: at least 5 timed repetitions")
    if a.child:
        print(json.dumps(measure(a.child, a.reps, a.warmup)))
        return 0
    out = {"tool": "tools/bench_tensor_layout.py", "reps": a.reps, "warmup": a.warmup,
           "metric": "ms per call sequence between device events; new = one call of this library with the option, old = the call without it + the torch "
                     "passes it replaces", "workloads": {}}
    for name in WORKLOADS:
        out["workloads"][name] = run_step(name, [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps),
                                                 "--warmup", str(a.warmup)], ROOT, 420)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    bad = []
    for name, w in out["workloads"].items():
        m = w["ms"]
        print("%-13s new %.3f ms (%.3f .. %.3f)   old %.3f ms (%.3f .. %.3f)   old / new %.3f   below by more than both spreads: %s   new == old: %s" % (
            name, m["new"]["median_ms"], m["new"]["min_ms"], m["new"]["max_ms"], m["old"]["median_ms"], m["old"]["min_ms"], m["old"]["max_ms"],
            m["old_over_new"], w["new_below_old_by_more_than_both_spreads"], w["new_equals_old_bit_for_bit"]))
        if not w["new_equals_old_bit_for_bit"] and name == "nhwc_resized":
            bad.append(name)
    print("wrote", a.out)
    if bad:
        raise SystemExit(f"the two variants differ on {bad}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
