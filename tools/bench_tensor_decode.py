#!/usr/bin/env python
"""Float tensors: does one decode_tensor call beat what a caller could do before it, and encode_f32 the conversion pass in front of encode_v?

  python tools/bench_tensor_decode.py [--reps 20] [--warmup 3] [--crop 384] [--out profiles/tensor_decode/bench.json]

Two workloads, natural-like images (llicti_amd/synth.py "smooth"), seed-1337 weights: 24 x 768x512 in container xrans15, and the first 24 sizes
of the reference's test set (tests/golden/eval_shapes.json, mixed) in container "auto".  The consumer wants a [24, 3, crop, crop] float16 tensor:
a random crop and a random horizontal flip per image (drawn once, seeded, the same for both legs), ImageNet mean / std.
  decode (A)  what the parent commit offers: decode_v into a flat uint8 buffer, then per image slice, / 255, normalise, flip, torch.stack, .half()
  decode (B)  ONE HipCodec.decode_tensor call writing that tensor (llicti_decode_images_tensor)
  encode (A)  LLICTI._to_u8 -- (x * 255).round().clamp_(0, 255).to(uint8) -- then encode_v
  encode (B)  HipCodec.encode_f32 on the float32 buffer (llicti_encode_images_f32)
Leg A divides by TENSORS (x / t255, / std): PyTorch turns a division by a Python scalar on the device into a product with the reciprocal, which
gives other bits.  Before anything is timed B is held against the arithmetic spec evaluated by PyTorch on the CPU (exact, or the run ends) and A
against B (recorded; a difference fails the run after the file is written); the containers of the two encode legs must be equal.
One round = A then B between device events on the compute stream, `--reps` rounds (at least 5) after `--warmup` untimed ones in ONE process, so
clock and temperature drift hit both alike; medians, min .. max and p10 .. p90 are reported.  `b_not_slower` asks for B's median <= A's median +
A's own min .. max spread.  Peak extra device memory of a leg: torch's allocator peak over one call minus what was allocated before it (B's
output is preallocated, so B's figure must be 0).  One profiled call of each leg gives kernel group "misc" (llicti_last_timing_detail): header /
unpack / init + the unlift of a decode, lift + min/max + header of an encode -- the only group the legs do not share.

The driver itself never touches the GPU: every workload is a child process under its own `timeout`, and the first one that fails ends the run.
"""
import argparse
import json
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


def workload_sizes(name):
    if name == "uniform":
        return [(512, 768)] * 24
    shapes = json.load(open(os.path.join(ROOT, "tests", "golden", "eval_shapes.json")))["shapes"]
    return [tuple(s) for s in shapes[:24]]


def pair(a, b):
    return {"a": a, "b": b, "b_minus_a_ms": round(b["median_ms"] - a["median_ms"], 4), "a_min_max_spread_ms": round(a["max_ms"] - a["min_ms"], 4),
            "b_not_slower": bool(b["median_ms"] <= a["median_ms"] + (a["max_ms"] - a["min_ms"]))}


def measure(name, reps, warmup, crop):
    """The child's work: one workload, decode legs and encode legs in one process; -> dict."""
    import numpy as np
    import torch
    from llicti_amd.codec import NSEG, HipCodec, auto_modes, mode_of_name, name_of_mode
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    from llicti_amd.synth import make_image
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1337)
    sd = LLICTI(default_config()).state_dict()
    sizes = workload_sizes(name)
    B = len(sizes)
    Hs, Ws = [h for h, _ in sizes], [w for _, w in sizes]
    assert min(Hs) >= crop and min(Ws) >= crop, "a crop must fit the smallest image"
    cache = {}
    imgs = []
    for i, (h, w) in enumerate(sizes):                   # (four distinct images per size are plenty: the generator is slow)
        key = (h, w, i % 4)
        if key not in cache:
            cache[key] = make_image("smooth", h, w, 100 + i % 4)
        imgs.append(cache[key])
    u8_host = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs]))
    c = HipCodec(dev)
    c.load_state_dict(sd)
    offs, total = c.flat_offsets(Hs, Ws)
    if name == "uniform":
        enc_mode = mode_of_name("xrans15")
    else:
        m = auto_modes(sizes)
        enc_mode = m[0] if all(v == m[0] for v in m) else m
    rng = np.random.default_rng(7)
    y0 = [int(rng.integers(0, h - crop + 1)) for h in Hs]
    x0 = [int(rng.integers(0, w - crop + 1)) for w in Ws]
    flip = [int(v) for v in rng.integers(0, 2, B)]
    mean_t = torch.tensor(MEAN, dtype=torch.float32, device=dev)[:, None, None]
    std_t = torch.tensor(STD, dtype=torch.float32, device=dev)[:, None, None]
    t255 = torch.tensor(255.0, dtype=torch.float32, device=dev)

    # ---- encode legs
    x_flat = (u8_host.float() / 255).to(dev)             # the caller's float32 buffer, {k/255} built on the CPU
    stride = max(c.max_container_bytes(h, w) for h, w in set(sizes))
    cont_a, seg_a = torch.empty((B, stride), dtype=torch.uint8, device=dev), torch.zeros((B, NSEG), dtype=torch.int32, device=dev)
    cont_b, seg_b = torch.empty_like(cont_a), torch.zeros_like(seg_a)

    def enc_a():
        return c.encode_v(LLICTI._to_u8(x_flat), Hs, Ws, enc_mode, out=cont_a, seg_len=seg_a)

    def enc_b():
        return c.encode_f32(x_flat, Hs, Ws, enc_mode, out=cont_b, seg_len=seg_b)
    enc_a()
    enc_b()
    c.check()
    assert torch.equal(seg_a, seg_b), "encode_f32: segment lengths differ from encode_v's"
    n = seg_a.sum(dim=1)
    assert all(torch.equal(cont_a[b, :int(n[b])], cont_b[b, :int(n[b])]) for b in range(B)), "encode_f32: container bytes differ from encode_v's"
    dm = c.container_modes(cont_a)
    dec_mode = dm[0] if all(v == dm[0] for v in dm) else dm

    # ---- decode legs
    flat_buf = torch.empty((total,), dtype=torch.uint8, device=dev)
    out_b = torch.empty((B, 3, crop, crop), dtype=torch.float16, device=dev)

    def dec_a():
        flat = c.decode_v(cont_a, seg_a, Hs, Ws, dec_mode, out=flat_buf)
        outs = []
        for b in range(B):
            win = flat[int(offs[b]):int(offs[b]) + 3 * Hs[b] * Ws[b]].view(3, Hs[b], Ws[b])[:, y0[b]:y0[b] + crop, x0[b]:x0[b] + crop]
            x = (win.float() / t255 - mean_t) / std_t
            outs.append(torch.flip(x, dims=[-1]) if flip[b] else x)
        return torch.stack(outs).to(torch.float16)

    def dec_b():
        return c.decode_tensor(cont_b, seg_b, Hs, Ws, dec_mode, size=(crop, crop), dtype=torch.float16, origin=(y0, x0), flip=flip,
                               mean=MEAN, std=STD, out=out_b)
    c.poison_workspace()
    got_a = dec_a()
    c.poison_workspace()
    got_b = dec_b().clone()
    c.check()
    # the spec on the CPU, from the original pixels (the codec is lossless)
    want = []
    for b, a in enumerate(imgs):
        win = torch.from_numpy(a)[:, y0[b]:y0[b] + crop, x0[b]:x0[b] + crop]
        x = (win.float() / 255 - mean_t.cpu()) / std_t.cpu()
        want.append(torch.flip(x, dims=[-1]) if flip[b] else x)
    want = torch.stack(want).to(torch.float16)
    assert torch.equal(got_b.cpu(), want), "decode_tensor differs from the arithmetic spec on the CPU"
    a_differs = int((got_a.view(torch.int16) != got_b.view(torch.int16)).sum())

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def peak_extra(fn):
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        r = fn()
        torch.cuda.synchronize(dev)
        peak = torch.cuda.max_memory_allocated(dev) - base
        del r
        return int(peak)
    cols = {"dec_a": [], "dec_b": [], "enc_a": [], "enc_b": []}
    legs = {"dec_a": dec_a, "dec_b": dec_b, "enc_a": enc_a, "enc_b": enc_b}
    for k in range(warmup + reps):
        t = {key: timed(fn) for key, fn in legs.items()}
        if k >= warmup:
            for key, v in t.items():
                cols[key].append(v)
    c.check()
    mem = {key: peak_extra(fn) for key, fn in legs.items()}
    counters = ("plan_builds", "plan_hits", "device_syncs", "device_allocs")
    before = {k: c.counter(k) for k in counters}
    for k in range(4):                                   # new windows every call: plan hits and nothing else
        c.decode_tensor(cont_b, seg_b, Hs, Ws, dec_mode, size=(crop, crop), dtype=torch.float16,
                        origin=([(v + k + 1) % (h - crop + 1) for v, h in zip(y0, Hs)], [(v + 3 * k + 1) % (w - crop + 1) for v, w in zip(x0, Ws)]),
                        flip=[(f + k) % 2 for f in flip], mean=MEAN, std=STD, out=out_b)
    after = {k: c.counter(k) for k in counters}
    c.set_profiling(True)
    prof = {}
    for key, fn in (("dec_a_decode_v", lambda: c.decode_v(cont_a, seg_a, Hs, Ws, dec_mode, out=flat_buf)), ("dec_b_decode_tensor", dec_b),
                    ("enc_a_encode_v", lambda: c.encode_v(flat_buf, Hs, Ws, enc_mode, out=cont_a, seg_len=seg_a)), ("enc_b_encode_f32", enc_b)):
        ms = []
        for _ in range(max(5, reps // 2)):
            fn()
            ms.append(c.last_timing_detail()[0]["misc"])
        prof[key] = {"misc_ms": stats(ms)}
    c.set_profiling(False)
    c.check()
    c.close()
    st = {k: stats(v) for k, v in cols.items()}
    modes = enc_mode if isinstance(enc_mode, list) else [enc_mode]
    return {"device": torch.cuda.get_device_name(dev), "images": B, "sizes": sorted({f"{w}x{h}" for h, w in sizes}),
            "megapixels": round(sum(h * w for h, w in sizes) / 1e6, 3), "container": sorted({name_of_mode(m) for m in modes}),
            "output": f"[{B}, 3, {crop}, {crop}] float16, random crop + flip per image, ImageNet mean / std",
            "decode_ms": pair(st["dec_a"], st["dec_b"]), "encode_ms": pair(st["enc_a"], st["enc_b"]),
            "peak_extra_device_bytes": mem, "b_allocates_nothing_besides_its_output": bool(mem["dec_b"] == 0),
            "decode_leg_a_elements_differing_from_b": a_differs,
            "four_calls_with_new_windows": {k: after[k] - before[k] for k in counters},
            "profiled_calls": prof}


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
    ap.add_argument("--crop", type=int, default=384, help="side of the square crop (it must fit the smallest image)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_decode", "bench.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.reps < 5:
        ap.error("--reps: at least 5 timed repetitions")
    if a.child:
        print(json.dumps(measure(a.child, a.reps, a.warmup, a.crop)))
        return 0
    out = {"tool": "tools/bench_tensor_decode.py", "reps": a.reps, "warmup": a.warmup,
           "metric": "ms per call sequence between device events; A = the parent commit's calls + torch passes, B = one call of this library",
           "workloads": {}}
    for name in ("uniform", "eval_shapes"):
        out["workloads"][name] = run_step(name, [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps),
                                                 "--warmup", str(a.warmup), "--crop", str(a.crop)], ROOT, 300)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    bad = []
    for name, w in out["workloads"].items():
        for leg in ("decode_ms", "encode_ms"):
            p = w[leg]
            print("%-12s %-9s A %.3f ms (min %.3f, max %.3f)   B %.3f ms (min %.3f, max %.3f)   b_not_slower: %s" % (
                name, leg[:-3], p["a"]["median_ms"], p["a"]["min_ms"], p["a"]["max_ms"], p["b"]["median_ms"], p["b"]["min_ms"], p["b"]["max_ms"],
                p["b_not_slower"]))
        print("%-12s peak extra device bytes %s; leg A elements differing from B: %d" % (name, w["peak_extra_device_bytes"],
                                                                                         w["decode_leg_a_elements_differing_from_b"]))
        if w["decode_leg_a_elements_differing_from_b"]:
            bad.append(name)
    print("wrote", a.out)
    if bad:
        raise SystemExit(f"decode leg A differs from leg B on {bad}: B equals the CPU spec, so A's device arithmetic is not the spec's")
    return 0


if __name__ == "__main__":
    sys.exit(main())
