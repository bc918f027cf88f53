#!/usr/bin/env python
"""Reduced-resolution decode: what stopping at level r saves, against the full decode of another build of the library.

  python tools/bench_reduce.py --parent-so /path/to/parent/libllicti_hip.so [--parent-src /path/to/parent/tree] [--parent-head HASH]
                               [--calls 24] [--warmup 4] [--out profiles/r9/reduced_decode.json]

Batches: bench.py's (24 x 768x512 uniform noise, seed-1337 weights), the natural-like one (24 x 768x512 smooth synthetic, trained-like weights of
tests/golden) and one 3840x2160 noise image; container "auto".  Metric: DECODE-ONLY time per call between two device events on the compute stream,
the containers already in HBM.  One round = the other build's full decode, then this build's r = 0 .. 5, so that clock and temperature drift hit
every column alike; `--calls` rounds after `--warmup` untimed ones.  Both libraries live in ONE process (two contexts on the same HIP runtime),
decode the SAME device containers, and every result is compared with the original's subsample before anything is timed.

Answers, from the numbers it has just measured (the JSON holds them all):
  full_decode_not_slower   this build's r = 0 median lies within the other build's own spread (10th .. 90th percentile) of its full decode
  r1_at_most_half          this build's r = 1 median <= half of the other build's full-decode median, on the 24-image batches
and, per r, one profiled call's kernel-group times (last_timing_detail) and band-CNN time per level (last_cnn_level_ms): where the time goes.
"""
import argparse
import ctypes as C
import glob
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sources_hash(tree):
    """sha256 over the library's sources of a tree (csrc/*.hip, *.hpp, include/llicti_hip.h), names included: which code a column measured."""
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(tree, "llicti_amd", "csrc", "*.h*"))) + [os.path.join(tree, "include", "llicti_hip.h")]
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()


def codec_of(so_path, dev):
    """A HipCodec on ANOTHER build of the library: bound like llicti_amd._lib.lib() binds its own (names the other build lacks are skipped)."""
    from llicti_amd import _lib
    from llicti_amd.codec import HipCodec
    import torch  # noqa: F401  (the HIP runtime both libraries bind to)
    L = C.CDLL(so_path)
    for name, (res, args) in _lib._SIGS.items():
        f = getattr(L, name, None)
        if f is not None:
            f.restype, f.argtypes = res, args
    own = _lib.lib()
    _lib._lib = L                       # (HipCodec takes the library from _lib.lib() once, when it is made)
    try:
        return HipCodec(dev)
    finally:
        _lib._lib = own


def stats(v):
    s = sorted(v)
    n = len(s)

    def pct(p):
        return s[min(n - 1, max(0, int(round(p * (n - 1)))))]
    return {"median_ms": round(statistics.median(s), 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4), "p10_ms": round(pct(0.1), 4),
            "p90_ms": round(pct(0.9), 4), "stdev_ms": round(statistics.pstdev(s), 4), "calls": n}


def smooth_batch(torch, dev, B, H, W):
    """bench.py natural_like_leg's content: low-pass noise + a gradient, generated on the GPU from a fixed seed."""
    g = torch.Generator(device=dev).manual_seed(2024)
    x = torch.randn((B, 3, H + 32, W + 32), device=dev, generator=g)
    k = torch.ones((3, 1, 9, 9), device=dev) / 81.0
    for _ in range(2):
        x = torch.nn.functional.conv2d(x, k, padding=4, groups=3)
    x = x[:, :, 16:16 + H, 16:16 + W]
    img = 128 + x[:, 0:1] * 900.0 + x * 250.0 + torch.linspace(-40, 40, W, device=dev)[None, None, None, :] + \
        torch.randn((B, 3, H, W), device=dev, generator=g) * 2.0
    return img.round().clamp(0, 255).to(torch.uint8).contiguous()


def run_batch(torch, dev, name, rgb, sd, parent_so, calls, warmup):
    import numpy as np
    from llicti_amd.codec import HipCodec, auto_modes, name_of_mode, reduced_dims
    B, _, H, W = rgb.shape
    new = HipCodec(dev)
    new.load_state_dict(sd)
    old = codec_of(parent_so, dev)
    old.load_state_dict(sd)
    enc_mode = auto_modes([(H, W)])[0]
    cont, seg = new.encode(rgb, mode=enc_mode)
    new.check()
    modes = sorted(set(new.container_modes(cont)))
    mode = modes[0] if len(modes) == 1 else new.container_modes(cont)
    Hs, Ws = [H] * B, [W] * B
    nlev = new.nlevels
    # correctness first, on poisoned workspaces
    old.workspace_v(Hs, Ws, mode)
    old.poison_workspace()
    rec_old = old.decode_v(cont, seg, Hs, Ws, mode).view(B, 3, H, W)
    old.check()
    assert torch.equal(rec_old, rgb), "the other build's full decode is not lossless"
    outs = {}
    for r in range(nlev + 1):
        new.workspace_v(Hs, Ws, mode)
        new.poison_workspace()
        hr, wr = reduced_dims(H, W, r)
        outs[r] = torch.empty((B * 3 * hr * wr,), dtype=torch.uint8, device=dev)
        new.decode_v(cont, seg, Hs, Ws, mode, out=outs[r], reduce=r)
        new.check()
        assert torch.equal(outs[r].view(B, 3, hr, wr), rgb[..., ::1 << r, ::1 << r]), f"reduce {r}: not the original's subsample"
    out_old = torch.empty_like(rgb).view(-1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    cols = {"parent_full": []}
    cols.update({f"r{r}": [] for r in range(nlev + 1)})
    for k in range(warmup + calls):
        t = {"parent_full": timed(lambda: old.decode_v(cont, seg, Hs, Ws, mode, out=out_old))}
        for r in range(nlev + 1):
            t[f"r{r}"] = timed(lambda: new.decode_v(cont, seg, Hs, Ws, mode, out=outs[r], reduce=r))
        if k >= warmup:
            for key, v in t.items():
                cols[key].append(v)
    new.check()
    old.check()
    res = {"workload": name, "B": B, "H": H, "W": W, "container": name_of_mode(enc_mode),
           "decoder_modes": [name_of_mode(m) for m in (mode if isinstance(mode, list) else [mode])],
           "bytes": int(seg.sum().item()), "bpp": round(8.0 * int(seg.sum().item()) / (B * H * W), 4),
           "sizes": {f"r{r}": "%dx%d" % reduced_dims(H, W, r)[::-1] for r in range(nlev + 1)},
           "decode_ms": {k: stats(v) for k, v in cols.items()}}
    # where the time goes: one profiled call per r (events around every kernel group: slower than the timed calls, read the shares)
    new.set_profiling(True)
    prof = {}
    for r in range(nlev + 1):
        new.decode_v(cont, seg, Hs, Ws, mode, out=outs[r], reduce=r)
        ms, n = new.last_timing()
        cat, per = new.last_timing_detail()
        prof[f"r{r}"] = {"call_ms": round(ms[0], 4), "cnn_launches": n, "groups_ms": {k: round(v, 4) for k, v in cat.items() if v > 0},
                         "cnn_level_ms": [round(v, 4) for v in new.last_cnn_level_ms()[:nlev]]}
    new.set_profiling(False)
    res["profiled_call"] = prof
    p, d = res["decode_ms"]["parent_full"], res["decode_ms"]
    res["r0_minus_parent_ms"] = round(d["r0"]["median_ms"] - p["median_ms"], 4)
    res["parent_spread_p10_p90_ms"] = round(p["p90_ms"] - p["p10_ms"], 4)
    res["full_decode_not_slower"] = bool(d["r0"]["median_ms"] <= p["p90_ms"])
    res["ratio_to_parent_full"] = {k: round(v["median_ms"] / p["median_ms"], 4) for k, v in d.items() if k != "parent_full"}
    res["r1_at_most_half"] = bool(d["r1"]["median_ms"] <= 0.5 * p["median_ms"])
    new.close()
    old.close()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-so", required=True, help="libllicti_hip.so of the build to compare with (its full decode is the yardstick)")
    ap.add_argument("--parent-src", default=None, help="source tree of that build (for its sources' hash)")
    ap.add_argument("--parent-head", default=None, help="commit of that build")
    ap.add_argument("--head", default=None, help="commit of this tree, if it has one")
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r9", "reduced_decode.json"))
    a = ap.parse_args(argv)
    if a.calls < 20:
        ap.error("--calls: at least 20 timed calls")
    import numpy as np
    import torch
    import bench
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1337)
    sd_rand = LLICTI(default_config()).state_dict()
    sd_tl = {k: v for k, v in np.load(os.path.join(ROOT, "tests", "golden", "weights_trainedlike.npz")).items()}
    out = {"tool": "tools/bench_reduce.py", "device": torch.cuda.get_device_name(dev), "calls": a.calls, "warmup": a.warmup,
           "metric": "decode-only ms per call between device events, containers in HBM; one round = parent full decode, then r = 0 .. 5",
           "heads": {"parent": a.parent_head, "parent_sources_sha256": sources_hash(a.parent_src) if a.parent_src else None,
                     "this": a.head, "this_sources_sha256": sources_hash(ROOT)},
           "batches": []}
    out["batches"].append(run_batch(torch, dev, "24x768x512 uniform noise (bench.py's batch), seed-1337 weights",
                                    torch.from_numpy(bench.make_batch(24, 512, 768, 0)).to(dev), sd_rand, a.parent_so, a.calls, a.warmup))
    out["batches"].append(run_batch(torch, dev, "24x768x512 smooth synthetic (bench.py's natural-like batch), trained-like weights",
                                    smooth_batch(torch, dev, 24, 512, 768), sd_tl, a.parent_so, a.calls, a.warmup))
    out["batches"].append(run_batch(torch, dev, "1x3840x2160 uniform noise, seed-1337 weights",
                                    torch.from_numpy(bench.make_batch(1, 2160, 3840, 77)).to(dev), sd_rand, a.parent_so, a.calls, a.warmup))
    big = out["batches"][:2]
    out["full_decode_not_slower"] = all(b["full_decode_not_slower"] for b in out["batches"])
    out["r1_at_most_half_of_parent_full_on_24_image_batches"] = all(b["r1_at_most_half"] for b in big)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for b in out["batches"]:
        d = b["decode_ms"]
        print(b["workload"])
        print("  parent full %.3f ms (p10 %.3f, p90 %.3f)" % (d["parent_full"]["median_ms"], d["parent_full"]["p10_ms"], d["parent_full"]["p90_ms"]))
        for r in range(6):
            print("  r=%d %-9s %.3f ms  x%.3f of parent full   cnn launches %d" % (r, b["sizes"][f"r{r}"], d[f"r{r}"]["median_ms"], b["ratio_to_parent_full"][f"r{r}"],
                                                                                  b["profiled_call"][f"r{r}"]["cnn_launches"]))
    print("full_decode_not_slower:", out["full_decode_not_slower"], " r1_at_most_half:", out["r1_at_most_half_of_parent_full_on_24_image_batches"])
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
