#!/usr/bin/env python
"""Views: does ONE decode_tensor_views call beat today's ways to several resized crops per image?

  python tools/bench_multi_view.py [--reps 20] [--warmup 3] [--out profiles/multi_view/bench.json]

24 natural-like images of 768x512 (llicti_amd/synth.py "smooth"), container "auto", seed-1337 weights, ImageNet mean / std, float16 outputs.
Boxes are drawn as torchvision's RandomResizedCrop draws them (tools/bench_resized_decode.py: random_resized_box, seeded), a random flip per
view; a draw the filter's scale limit of 4 would refuse at reduce 0 is drawn again.  reduce is what codec.multi_crop_plan picks.
  workload "two_views"   two 224x224 views per image at scale 0.08 .. 1: one group of 48 views
  workload "multi_crop"  two 224x224 views at scale 0.4 .. 1 and six 96x96 views at scale 0.05 .. 0.4 per image: two groups, 48 and 144 views
  variant i    the new call: one HipCodec.decode_tensor_views (llicti_decode_images_tensor_views) -- one decode, one last-kernel pass per view
  variant ii   today's way to the same bytes: one decode_tensor_resized call per view index on the whole batch (2 and 8 calls, as many decodes)
  variant iii  today's one-decode way: decode_v at full size, then per view slice, F.interpolate(bilinear, antialias=True), / 255, normalise,
               flip; torch.stack and .half() per group
One round = i, ii, iii between device events on the compute stream; `--reps` rounds (at least 5) after `--warmup` untimed ones of every variant
in ONE process, so clock and temperature drift hit all alike; medians and min .. max are reported.  i must equal ii bit for bit on the timed
inputs, or the run fails after the file is written.  i against iii: the largest difference is recorded (at reduce 0 the same filter in two
fp32 orders; at reduce >= 1 variant i resamples a decimated image: different pictures).  Against ii the file records whether i's median lies
below ii's by more than the two spreads (max - min) added together; against iii it only reports.

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

# workload -> [(output side, views per image, scale range)]
WORKLOADS = {"two_views": [(224, 2, (0.08, 1.0))], "multi_crop": [(224, 2, (0.4, 1.0)), (96, 6, (0.05, 0.4))]}


def measure(name, reps, warmup):
    """The child's work: one workload, the three variants in one process; -> dict."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    from llicti_amd.codec import HipCodec, auto_modes, multi_crop_plan, name_of_mode
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    from llicti_amd.synth import make_image
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1337)
    sd = LLICTI(default_config()).state_dict()
    B, H, W, distinct = 24, 512, 768, 4                   # (the generator is slow: four distinct images)
    sizes = [(H, W)] * B
    Hs, Ws = [H] * B, [W] * B
    rng = np.random.default_rng(11)
    # views in view-major order: view k of image b is entry k * B + b of its group, so variant ii's call k writes one contiguous slice
    spec, full = [], []
    for side, per, scale in WORKLOADS[name]:
        image, boxes = [], []
        for _k in range(per):
            for b in range(B):
                box = random_resized_box(rng, H, W, scale=scale)
                while box[2] > 4 * side or box[3] > 4 * side:
                    box = random_resized_box(rng, H, W, scale=scale)
                image.append(b)
                boxes.append(box)
        spec.append(dict(side=side, per=per, image=image, flip=[int(v) for v in rng.integers(0, 2, len(image))]))
        full.append(((side, side), image, boxes))
    reduce, mapped = multi_crop_plan(sizes, full)
    made = [make_image("smooth", H, W, 100 + i) for i in range(distinct)]
    c = HipCodec(dev)
    c.load_state_dict(sd)
    offs, total = c.flat_offsets(Hs, Ws)
    m = auto_modes(sizes)
    enc_mode = m[0] if all(v == m[0] for v in m) else m
    cont, seg = c.encode_v(torch.from_numpy(np.concatenate([made[i % distinct].reshape(-1) for i in range(B)])).to(dev), Hs, Ws, enc_mode)
    c.check()
    dm = c.container_modes(cont)
    assert all(v == dm[0] for v in dm)                    # (equal sizes: one mode)
    dec_mode = dm[0]
    mean_t = torch.tensor(MEAN, dtype=torch.float32, device=dev)[:, None, None]
    std_t = torch.tensor(STD, dtype=torch.float32, device=dev)[:, None, None]
    t255 = torch.tensor(255.0, dtype=torch.float32, device=dev)
    flat_buf = torch.empty((total,), dtype=torch.uint8, device=dev)
    out_i = [torch.empty((len(s["image"]), 3, s["side"], s["side"]), dtype=torch.float16, device=dev) for s in spec]
    out_ii = [torch.empty_like(o) for o in out_i]
    groups = [dict(size=(s["side"], s["side"]), image=s["image"], boxes=bx, flip=s["flip"], dtype=torch.float16, antialias=True, out=o)
              for s, bx, o in zip(spec, mapped, out_i)]

    def var_i():
        return c.decode_tensor_views(cont, seg, Hs, Ws, dec_mode, groups, mean=MEAN, std=STD, reduce=reduce)

    def var_ii():
        for s, bx, o in zip(spec, mapped, out_ii):
            for k in range(s["per"]):
                c.decode_tensor_resized(cont, seg, Hs, Ws, dec_mode, (s["side"], s["side"]), bx[k * B:(k + 1) * B], dtype=torch.float16,
                                        flip=s["flip"][k * B:(k + 1) * B], mean=MEAN, std=STD, antialias=True, reduce=reduce, out=o[k * B:(k + 1) * B])
        return out_ii

    def var_iii():
        flat = c.decode_v(cont, seg, Hs, Ws, dec_mode, out=flat_buf)
        res = []
        for s, (_, image, boxes) in zip(spec, full):
            outs = []
            for b, (y0, x0, h, w), fl in zip(image, boxes, s["flip"]):
                win = flat[int(offs[b]):int(offs[b]) + 3 * H * W].view(3, H, W)[:, y0:y0 + h, x0:x0 + w]
                x = F.interpolate(win.float()[None], size=(s["side"], s["side"]), mode="bilinear", align_corners=False, antialias=True)[0]
                x = (x / t255 - mean_t) / std_t
                outs.append(torch.flip(x, dims=[-1]) if fl else x)
            res.append(torch.stack(outs).to(torch.float16))
        return res
    c.poison_workspace()
    got_iii = var_iii()
    c.poison_workspace()
    var_ii()
    c.poison_workspace()
    var_i()
    c.check()
    equal = [bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8))) for a, b in zip(out_i, out_ii)]
    diff = [float((a.float() - b.float()).abs().max()) for a, b in zip(out_i, got_iii)]

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    cols = {"i": [], "ii": [], "iii": []}
    for k in range(warmup + reps):
        t = {"i": timed(var_i), "ii": timed(var_ii), "iii": timed(var_iii)}
        if k >= warmup:
            for key, v in t.items():
                cols[key].append(v)
    c.check()
    equal_after = [bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8))) for a, b in zip(out_i, out_ii)]
    counters = ("plan_builds", "plan_hits", "device_syncs", "device_allocs")
    before = {k: c.counter(k) for k in counters}
    for _ in range(4):                                    # new views every call: plan hits and nothing else
        fresh = []
        for g, s in zip(groups, spec):
            bx = []
            for b in s["image"]:
                y0, x0, h, w = random_resized_box(rng, H, W)
                bx.append((y0 >> reduce, x0 >> reduce, max(1, min(h >> reduce, 4 * s["side"])), max(1, min(w >> reduce, 4 * s["side"]))))
            fresh.append(dict(g, boxes=bx, flip=[int(v) for v in rng.integers(0, 2, len(bx))]))
        c.decode_tensor_views(cont, seg, Hs, Ws, dec_mode, fresh, mean=MEAN, std=STD, reduce=reduce)
    after = {k: c.counter(k) for k in counters}
    c.set_profiling(True)
    prof = {}
    for key, fn in (("i_decode_tensor_views", var_i), ("one_decode_tensor_resized", lambda: c.decode_tensor_resized(
            cont, seg, Hs, Ws, dec_mode, (spec[0]["side"],) * 2, mapped[0][:B], dtype=torch.float16, mean=MEAN, std=STD, reduce=reduce, out=out_ii[0][:B]))):
        fn()
        cat, per = c.last_timing_detail()
        prof[key] = {"band_cnn_launches": len(per), "kernel_group_ms": {k: round(v, 4) for k, v in cat.items()}}
    c.set_profiling(False)
    c.check()
    c.close()
    st = {k: stats(v) for k, v in cols.items()}
    spread = {k: round(v["max_ms"] - v["min_ms"], 4) for k, v in st.items()}
    gain = round(st["ii"]["median_ms"] - st["i"]["median_ms"], 4)
    modes = enc_mode if isinstance(enc_mode, list) else [enc_mode]
    return {"device": torch.cuda.get_device_name(dev), "images": B, "sizes": [f"{W}x{H}"], "container": sorted({name_of_mode(v) for v in modes}),
            "groups": [{"output": f"[{len(s['image'])}, 3, {s['side']}, {s['side']}] float16", "views_per_image": s["per"]} for s in spec],
            "reduce": reduce, "calls_of_variant_ii": sum(s["per"] for s in spec),
            "ms": {**st, "spread_ms": spread, "ii_minus_i_ms": gain, "ii_over_i": round(st["ii"]["median_ms"] / st["i"]["median_ms"], 3),
                   "iii_over_i": round(st["iii"]["median_ms"] / st["i"]["median_ms"], 3)},
            "i_below_ii_by_more_than_both_spreads": bool(gain > spread["i"] + spread["ii"]),
            "i_equals_ii_bit_for_bit": bool(all(equal) and all(equal_after)), "max_abs_difference_i_iii_per_group": diff,
            "difference_note": "reduce = 0: the same filter in two fp32 orders, rounded to float16; reduce >= 1: variant i resamples a decimated "
            "image, variant iii low-passes the full one -- they are different pictures",
            "four_calls_with_new_views": {k: after[k] - before[k] for k in counters}, "profiled_calls": prof}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_view", "bench.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.reps < 5:
        ap.error("--reps: at least 5 timed repetitions")
    if a.child:
        print(json.dumps(measure(a.child, a.reps, a.warmup)))
        return 0
    out = {"tool": "tools/bench_multi_view.py", "reps": a.reps, "warmup": a.warmup,
           "metric": "ms per call sequence between device events; i = one decode_tensor_views call, ii = one decode_tensor_resized call per view "
                     "index, iii = decode_v + torch passes per view", "workloads": {}}
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
        print("%-10s reduce %d   i %.3f ms (%.3f .. %.3f)   ii %.3f ms (%.3f .. %.3f)   iii %.3f ms (%.3f .. %.3f)   ii / i %.2f   below by more than both "
              "spreads: %s   i == ii: %s   max |i - iii| %s" % (
                  name, w["reduce"], m["i"]["median_ms"], m["i"]["min_ms"], m["i"]["max_ms"], m["ii"]["median_ms"], m["ii"]["min_ms"], m["ii"]["max_ms"],
                  m["iii"]["median_ms"], m["iii"]["min_ms"], m["iii"]["max_ms"], m["ii_over_i"], w["i_below_ii_by_more_than_both_spreads"],
                  w["i_equals_ii_bit_for_bit"], w["max_abs_difference_i_iii_per_group"]))
        if not w["i_equals_ii_bit_for_bit"]:
            bad.append(name)
    print("wrote", a.out)
    if bad:
        raise SystemExit(f"variant i differs from variant ii on {bad}: the views are not decode_tensor_resized's bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
