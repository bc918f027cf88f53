#!/usr/bin/env python
"""Per-image reduce: what does ONE call in which every image stops at its own level cost, against the ways a loader has without it?

  python tools/bench_per_image_reduce.py [--reps 20] [--warmup 3] [--size 224] [--out profiles/per_image_reduce/bench.json]

Natural-like images (llicti_amd/synth.py "smooth"), seed-1337 weights, container "auto".  Every image gets a box drawn as torchvision's
RandomResizedCrop draws it (tools/bench_resized_decode.py: random_resized_box, seeded) and a random flip; ImageNet mean / std; the output is the
[B, 3, size, size] float16 batch tensor.  resized_crop_plan(..., per_image=True) gives image b the largest r_b at which its own box keeps
size x size decoded pixels.
  workload "uhd"    8 x 3840x2160, the boxes of tools/bench_resized_decode.py's "uhd" (the same seed).  Three legs:
      grouped   that tool's leg B, the parent's way: the batch sorted into groups of equal reduce up front, one decode_tensor_resized call per group
      rv        ONE decode_tensor_resized(reduce=[r_b]) call, the batch in the loader's order
      scalar    the one call at reduce = min r_b -- with antialias=True, or antialias=False if the library refuses that (boxes that shrink by
                more than 4); the file says which
  workload "photo"  24 images at sizes drawn from 1024x768 .. 2048x1536 (seeded; the first seed from 1 on whose boxes force r = 0 for at least one
                    image and leave r >= 1 to at least a third).  Two legs: scalar (the call at the common reduce, as above) and rv.
One round = every leg once between device events on the compute stream, `--reps` rounds (at least 5) after `--warmup` untimed ones in ONE
process; medians and min .. max.  Per leg the file also holds last_cnn_level_ms and the band-CNN launch count (profiling on, one more run), the
host time of a call (perf_counter around the enqueue, no synchronisation inside) and the legs' largest difference; for rv the counters
device_syncs / device_allocs / plan_builds over four more calls with fresh boxes AND reduces.  No speed target is set.

The driver itself never touches the GPU: every workload is a child process under its own `timeout`, and the first one that fails ends the run.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_resized_decode import MEAN, STD, random_resized_box, run_step, stats  # noqa: E402

COUNTERS = ("plan_builds", "plan_hits", "device_syncs", "device_allocs")


def photo_draw(size):
    """-> (seed, sizes, full-resolution boxes, flips, r_b): the first seed whose batch has an image that needs level 0 and a third that do not"""
    import numpy as np
    from llicti_amd.codec import resized_crop_plan
    for seed in range(1, 200):
        rng = np.random.default_rng(seed)
        sizes = []
        for _ in range(24):
            w = int(rng.integers(1024, 2049))
            sizes.append((w * 3 // 4, w))
        full = [random_resized_box(rng, h, w) for h, w in sizes]
        flip = [int(v) for v in rng.integers(0, 2, len(sizes))]
        own = resized_crop_plan(sizes, full, (size, size), per_image=True)[0]
        if min(own) == 0 and 3 * sum(r >= 1 for r in own) >= len(own):
            return seed, sizes, full, flip, own
    raise SystemExit("photo: no seed below 200 gives the batch the workload asks for")


def measure(name, reps, warmup, size):
    """The child's work: one workload, its legs in one process; -> dict."""
    import numpy as np
    import torch
    from llicti_amd._lib import EINVAL, LlictiError
    from llicti_amd.codec import HipCodec, auto_modes, name_of_mode, resized_crop_plan
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    from llicti_amd.synth import make_image
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1337)
    sd = LLICTI(default_config()).state_dict()
    if name == "uhd":
        sizes = [(2160, 3840)] * 8
        rng = np.random.default_rng(7)
        full = [random_resized_box(rng, h, w) for h, w in sizes]
        flip = [int(v) for v in rng.integers(0, 2, len(sizes))]
        own = resized_crop_plan(sizes, full, (size, size), per_image=True)[0]
        seed = 7
        made = [make_image("smooth", 2160, 3840, 100 + i) for i in range(2)]              # (the generator is slow)
    else:
        seed, sizes, full, flip, own = photo_draw(size)
        rng = np.random.default_rng(1000 + seed)
        made = [make_image("smooth", 1536, 2048, 100 + i) for i in range(3)]
    B = len(sizes)
    Hs, Ws = [h for h, _ in sizes], [w for _, w in sizes]
    imgs = [np.ascontiguousarray(made[i % len(made)][:, :h, :w]) for i, (h, w) in enumerate(sizes)]
    c = HipCodec(dev)
    c.load_state_dict(sd)
    m = auto_modes(sizes)
    cont, seg = c.encode_v(torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(dev), Hs, Ws, m[0] if all(v == m[0] for v in m) else m)
    c.check()
    dm = c.container_modes(cont)
    mode = dm[0] if all(v == dm[0] for v in dm) else dm
    kw = dict(dtype=torch.float16, mean=MEAN, std=STD)

    # rv: the loader's order, every image at its own r
    boxes_rv = resized_crop_plan(sizes, full, (size, size), per_image=True)[1]
    out_rv = torch.empty((B, 3, size, size), dtype=torch.float16, device=dev)

    def leg_rv(rs=own, bx=boxes_rv):
        return c.decode_tensor_resized(cont, seg, Hs, Ws, mode, (size, size), bx, flip=flip, antialias=True, reduce=rs, out=out_rv, **kw)

    # scalar: the one call at the common reduce, in whichever form the library takes it
    rmin, boxes_min = resized_crop_plan(sizes, full, (size, size))
    assert rmin == min(own)
    out_sc = torch.empty_like(out_rv)
    scalar_antialias = True
    try:
        c.decode_tensor_resized(cont, seg, Hs, Ws, mode, (size, size), boxes_min, flip=flip, antialias=True, reduce=rmin, out=out_sc, **kw)
        refusal = None
    except LlictiError as e:
        if e.code != EINVAL:
            raise
        scalar_antialias, refusal = False, str(e)

    def leg_scalar():
        return c.decode_tensor_resized(cont, seg, Hs, Ws, mode, (size, size), boxes_min, flip=flip, antialias=scalar_antialias, reduce=rmin, out=out_sc, **kw)

    legs = {"rv": leg_rv, "scalar": leg_scalar}
    order = sorted(range(B), key=lambda b: own[b])
    if name == "uhd":
        # grouped: the batch in group order up front (every group reads and writes one contiguous slice), one call per reduce
        idx = torch.as_tensor(order, device=dev)
        g_cont, g_seg = cont[idx].contiguous(), seg[idx].contiguous()
        g_own, g_full, g_flip = [own[b] for b in order], [full[b] for b in order], [flip[b] for b in order]
        g_mode = mode if not isinstance(mode, list) else [mode[b] for b in order]
        groups, g_boxes = [], []
        for r in sorted(set(g_own)):
            lo, hi = g_own.index(r), B - g_own[::-1].index(r)
            groups.append((r, lo, hi))
            g_boxes += resized_crop_plan(sizes[lo:hi], g_full[lo:hi], (size, size))[1]
        out_g = torch.empty_like(out_rv)

        def leg_grouped():
            for r, lo, hi in groups:
                c.decode_tensor_resized(g_cont[lo:hi], g_seg[lo:hi], Hs[lo:hi], Ws[lo:hi], g_mode if not isinstance(g_mode, list) else g_mode[lo:hi], (size, size),
                                        g_boxes[lo:hi], flip=g_flip[lo:hi], antialias=True, reduce=r, out=out_g[lo:hi], **kw)
            return out_g
        legs = {"grouped": leg_grouped, **legs}

    # once, on a poisoned workspace: the tensors
    got = {}
    for key, fn in legs.items():
        c.poison_workspace()
        got[key] = fn().clone()
        c.check()
    diffs = {"rv_vs_scalar": float((got["rv"].float() - got["scalar"].float()).abs().max())}
    if name == "uhd":
        diffs["rv_vs_grouped"] = float((got["rv"][torch.as_tensor(order, device=dev)].float() - got["grouped"].float()).abs().max())

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cols, host = {k: [] for k in legs}, {k: [] for k in legs}
    for k in range(warmup + reps):
        for key, fn in legs.items():
            e0.record()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            if k >= warmup:
                cols[key].append(e0.elapsed_time(e1))
                host[key].append((t1 - t0) * 1e3)
    c.check()

    # four more rv calls, fresh boxes AND reduces each
    before = {k: c.counter(k) for k in COUNTERS}
    fresh_reduces = []
    for _ in range(4):
        fb = [random_resized_box(rng, h, w) for h, w in sizes]
        rs, bx = resized_crop_plan(sizes, fb, (size, size), per_image=True)
        if len(set(rs)) == 1:
            continue
        fresh_reduces.append(rs)
        leg_rv(rs, bx)
    after = {k: c.counter(k) for k in COUNTERS}
    c.check()

    c.set_profiling(True)
    prof = {}
    for key in legs:
        lev, launches, cat = [0.0] * 5, 0, {}
        if key == "grouped":
            for r, lo, hi in groups:
                c.decode_tensor_resized(g_cont[lo:hi], g_seg[lo:hi], Hs[lo:hi], Ws[lo:hi], g_mode if not isinstance(g_mode, list) else g_mode[lo:hi], (size, size),
                                        g_boxes[lo:hi], flip=g_flip[lo:hi], antialias=True, reduce=r, out=out_g[lo:hi], **kw)
                lev = [a + b for a, b in zip(lev, c.last_cnn_level_ms())]
                d, per = c.last_timing_detail()
                launches += len(per)
                cat = {k: cat.get(k, 0.0) + v for k, v in d.items()}
        else:
            legs[key]()
            lev = c.last_cnn_level_ms()
            cat, per = c.last_timing_detail()
            launches = len(per)
        prof[key] = {"last_cnn_level_ms": [round(v, 4) for v in lev], "band_cnn_launches": launches, "kernel_group_ms": {k: round(v, 4) for k, v in cat.items()}}
    c.set_profiling(False)
    c.check()
    c.close()

    ms = {k: stats(v) for k, v in cols.items()}
    res = {"device": torch.cuda.get_device_name(dev), "images": B, "sizes": sorted({f"{w}x{h}" for h, w in sizes}), "seed": seed,
           "megapixels": round(sum(h * w for h, w in sizes) / 1e6, 3), "container": sorted({name_of_mode(v) for v in (mode if isinstance(mode, list) else [mode])}),
           "output": f"[{B}, 3, {size}, {size}] float16, random resized crop + flip per image, ImageNet mean / std",
           "boxes_full_resolution_yxhw": [list(v) for v in full], "reduces": own, "images_that_skip_level_0": sum(r >= 1 for r in own),
           "scalar_call": {"reduce": rmin, "antialias": scalar_antialias, "refusal_with_antialias": refusal},
           "ms": ms, "host_ms_per_call_sequence": {k: round(statistics.median(v), 4) for k, v in host.items()},
           "rv_over_scalar": round(ms["rv"]["median_ms"] / ms["scalar"]["median_ms"], 3),
           "max_abs_difference": diffs,
           "difference_note": "rv against grouped: the same decodes, put in the same order -- 0 is expected; rv against scalar: the scalar call resamples "
                              "every image from the finest common grid (and without the filter where that is how it was accepted): different pictures",
           "four_rv_calls_with_fresh_boxes_and_reduces": {"reduces": fresh_reduces, **{k: after[k] - before[k] for k in COUNTERS}},
           "profiled_calls": prof}
    if name == "uhd":
        res["calls_of_leg_grouped"] = [{"reduce": r, "images": hi - lo} for r, lo, hi in groups]
        res["rv_minus_grouped_ms"] = round(ms["rv"]["median_ms"] - ms["grouped"]["median_ms"], 4)
        res["grouped_spread_ms"] = round(ms["grouped"]["max_ms"] - ms["grouped"]["min_ms"], 4)
    else:
        l0 = {k: prof[k]["last_cnn_level_ms"][0] for k in ("scalar", "rv")}
        res["level0_cnn_ms"] = {**l0, "rv_over_scalar": round(l0["rv"] / l0["scalar"], 3) if l0["scalar"] > 0 else None,
                                "share_of_level0_pixels_rv_decodes": round(sum(h * w for (h, w), r in zip(sizes, own) if r == 0) / sum(h * w for h, w in sizes), 3)}
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=224, help="side of the square output")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "per_image_reduce", "bench.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.reps < 5:
        ap.error("--reps: at least 5 timed repetitions")
    if a.child:
        print(json.dumps(measure(a.child, a.reps, a.warmup, a.size)))
        return 0
    out = {"tool": "tools/bench_per_image_reduce.py", "reps": a.reps, "warmup": a.warmup,
           "metric": "ms per call sequence between device events, every leg once per round; medians, min .. max", "workloads": {}}
    for name in ("uhd", "photo"):
        out["workloads"][name] = run_step(name, [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps),
                                                 "--warmup", str(a.warmup), "--size", str(a.size)], ROOT, 420)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for name, w in out["workloads"].items():
        print("%-6s reduces %s" % (name, w["reduces"]))
        for key, m in w["ms"].items():
            print("   %-8s %.3f ms (min %.3f, max %.3f)   host %.3f ms   CNN launches %d   level-0 CNN %.3f ms" % (
                key, m["median_ms"], m["min_ms"], m["max_ms"], w["host_ms_per_call_sequence"][key], w["profiled_calls"][key]["band_cnn_launches"],
                w["profiled_calls"][key]["last_cnn_level_ms"][0]))
        print("   scalar call: reduce %d, antialias %s; max |rv - .|: %s; fresh calls: %s" % (
            w["scalar_call"]["reduce"], w["scalar_call"]["antialias"], w["max_abs_difference"],
            {k: v for k, v in w["four_rv_calls_with_fresh_boxes_and_reduces"].items() if k != "reduces"}))
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
