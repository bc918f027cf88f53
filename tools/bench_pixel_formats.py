#!/usr/bin/env python
"""Interleaved pixel buffers: do the new calls beat what a caller could do before them?

  python tools/bench_pixel_formats.py [--reps 10] [--warmup 3] [--parent-tree /path/to/parent/checkout] [--bench-steps 5]
                                      [--out profiles/pixel_formats/bench.json]

The batch is bench.py's: 24 x 768x512 uniform noise, seed-1337 weights, container "auto".  Both contenders start from an interleaved RGB8 device
buffer and end in one:
  (a) permute    x.permute(0, 3, 1, 2).contiguous() on the device, the planar encode, the planar decode, .permute(0, 2, 3, 1).contiguous()
                 -- everything a caller of the parent commit can do without a host transpose;
  (b) px         HipCodec.encode_px, HipCodec.decode_px (llicti_encode_images_px / llicti_decode_images_px): no extra pass.
One round = (a) then (b), timed between device events on the compute stream, output buffers allocated once; `--reps` rounds (at least 5) after
`--warmup` untimed ones, in ONE process, so that clock and temperature drift hit both alike.  Medians and the p10 .. p90 spread are reported;
(b) moves strictly fewer bytes, so `px_not_slower` asks for (b)'s median <= (a)'s median and states both spreads beside it.  Both results are
compared with the input before anything is timed.  One profiled call of each of the four codec calls gives the kernel-group times
(llicti_last_timing_detail): group "misc" holds the lift (+ min/max + header) of an encode and the header / unpack / unlift of a decode, the only
groups the two paths do not share.

The driver itself never touches the GPU: every GPU step is a child process under its own `timeout`, and the first step that fails ends the run.
Steps: the measurement above; `bench.py --gpus 1` of this tree (the planar headline on the same build); with --parent-tree, `bench.py --gpus 1`
of that tree (built there beforehand) -- the planar path launches unchanged code, so the two headlines must agree within their run-to-run spread.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    s = sorted(v)
    n = len(s)

    def pct(p):
        return s[min(n - 1, max(0, int(round(p * (n - 1)))))]
    return {"median_ms": round(statistics.median(s), 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4), "p10_ms": round(pct(0.1), 4),
            "p90_ms": round(pct(0.9), 4), "reps": n}


def measure(reps, warmup):
    """The child's work: (a) against (b) in one process; -> dict."""
    import torch
    import bench
    from llicti_amd.codec import NSEG, HipCodec, auto_modes, name_of_mode
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1337)
    sd = LLICTI(default_config()).state_dict()
    B, H, W = 24, 512, 768
    rgb = torch.from_numpy(bench.make_batch(B, H, W, 0)).to(dev)
    pix = rgb.permute(0, 2, 3, 1).contiguous().view(-1)                 # the caller's buffer: interleaved RGB8, tight
    c = HipCodec(dev)
    c.load_state_dict(sd)
    enc_mode = auto_modes([(H, W)])[0]
    Hs, Ws = [H] * B, [W] * B
    stride = c.max_container_bytes(H, W)
    cont_a, seg_a = torch.empty((B, stride), dtype=torch.uint8, device=dev), torch.zeros((B, NSEG), dtype=torch.int32, device=dev)
    cont_b, seg_b = torch.empty_like(cont_a), torch.zeros_like(seg_a)
    rec_a = torch.empty((B, 3, H, W), dtype=torch.uint8, device=dev)
    out_b = torch.empty_like(pix)
    # correctness first: same containers, both decodes give the input back
    c.encode(pix.view(B, H, W, 3).permute(0, 3, 1, 2).contiguous(), mode=enc_mode, out=cont_a, seg_len=seg_a)
    c.encode_px(pix, Hs, Ws, enc_mode, "rgb", out=cont_b, seg_len=seg_b)
    c.check()
    assert torch.equal(seg_a, seg_b), "px encode: segment lengths differ from the planar encode's"
    n = seg_a.sum(dim=1)
    assert all(torch.equal(cont_a[b, :int(n[b])], cont_b[b, :int(n[b])]) for b in range(B)), "px encode: container bytes differ from the planar encode's"
    dm = c.container_modes(cont_a)
    dec_mode = dm[0] if all(m == dm[0] for m in dm) else dm
    c.poison_workspace()
    out_a = c.decode_v(cont_a, seg_a, Hs, Ws, dec_mode, out=rec_a.view(-1)).view(B, 3, H, W).permute(0, 2, 3, 1).contiguous().view(-1)
    c.poison_workspace()
    c.decode_px(cont_b, seg_b, Hs, Ws, dec_mode, "rgb", out=out_b)
    c.check()
    assert torch.equal(out_a, pix) and torch.equal(out_b, pix), "round trip is not lossless"

    def path_a():
        x = pix.view(B, H, W, 3).permute(0, 3, 1, 2).contiguous()
        c.encode(x, mode=enc_mode, out=cont_a, seg_len=seg_a)
        c.decode_v(cont_a, seg_a, Hs, Ws, dec_mode, out=rec_a.view(-1))
        return rec_a.permute(0, 2, 3, 1).contiguous()

    def path_b():
        c.encode_px(pix, Hs, Ws, enc_mode, "rgb", out=cont_b, seg_len=seg_b)
        return c.decode_px(cont_b, seg_b, Hs, Ws, dec_mode, "rgb", out=out_b)

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    cols = {"permute": [], "px": []}
    for k in range(warmup + reps):
        t = {"permute": timed(path_a), "px": timed(path_b)}
        if k >= warmup:
            for key, v in t.items():
                cols[key].append(v)
    c.check()
    # the two transposes of (a) on their own
    perm = {"to_planar": [], "to_interleaved": []}
    for k in range(warmup + reps):
        t = {"to_planar": timed(lambda: pix.view(B, H, W, 3).permute(0, 3, 1, 2).contiguous()),
             "to_interleaved": timed(lambda: rec_a.permute(0, 2, 3, 1).contiguous())}
        if k >= warmup:
            for key, v in t.items():
                perm[key].append(v)
    # kernel groups of one profiled call each ("misc": lift + min/max + header of an encode; header / unpack / init + unlift of a decode)
    c.set_profiling(True)
    prof = {}
    x = pix.view(B, H, W, 3).permute(0, 3, 1, 2).contiguous()
    for name, fn in (("planar_encode", lambda: c.encode(x, mode=enc_mode, out=cont_a, seg_len=seg_a)),
                     ("px_encode", lambda: c.encode_px(pix, Hs, Ws, enc_mode, "rgb", out=cont_b, seg_len=seg_b)),
                     ("planar_decode", lambda: c.decode_v(cont_a, seg_a, Hs, Ws, dec_mode, out=rec_a.view(-1))),
                     ("px_decode", lambda: c.decode_px(cont_b, seg_b, Hs, Ws, dec_mode, "rgb", out=out_b))):
        ms = []
        for _ in range(max(5, reps)):
            fn()
            ms.append(c.last_timing_detail()[0]["misc"])
        prof[name] = {"misc_ms": stats(ms)}
    c.set_profiling(False)
    c.check()
    c.close()
    a, b = stats(cols["permute"]), stats(cols["px"])
    mpix = B * H * W / 1e6
    return {"device": torch.cuda.get_device_name(dev), "workload": f"{B}x{W}x{H} uniform noise (bench.py's batch), seed-1337 weights, interleaved RGB8 in HBM",
            "container": name_of_mode(enc_mode), "reps": reps, "warmup": warmup,
            "metric": "ms per encode + decode between device events, from an interleaved RGB8 device buffer back into one",
            "permute_path_ms": a, "px_path_ms": b,
            "permute_path_mpix_s": round(mpix / a["median_ms"] * 1e3, 1), "px_path_mpix_s": round(mpix / b["median_ms"] * 1e3, 1),
            "px_minus_permute_ms": round(b["median_ms"] - a["median_ms"], 4),
            "spread_p10_p90_ms": {"permute": round(a["p90_ms"] - a["p10_ms"], 4), "px": round(b["p90_ms"] - b["p10_ms"], 4)},
            "px_not_slower": bool(b["median_ms"] <= a["median_ms"]),
            "transposes_alone_ms": {k: stats(v) for k, v in perm.items()},
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


def headline(line):
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "bpp")
    return {k: line[k] for k in keep if k in line}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=5, help="bench.py --steps of the headline runs (0: skip them)")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its bench.py headline is recorded beside this tree's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_formats", "bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.reps < 5:
        ap.error("--reps: at least 5 timed repetitions")
    if a.child:
        print(json.dumps(measure(a.reps, a.warmup)))
        return 0
    out = {"tool": "tools/bench_pixel_formats.py"}
    out.update(run_step("permute path against px path", [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup", str(a.warmup)],
                        ROOT, 300))
    if a.bench_steps > 0:
        flags = ["--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "2", "--no-cpu-baseline", "--no-extras", "--no-pcie-legs", "--no-ac-leg"]
        out["bench_py_headline"] = {"this_tree": headline(run_step("bench.py, this tree", [sys.executable, "bench.py"] + flags, ROOT, 420))}
        if a.parent_tree:
            out["bench_py_headline"]["parent_tree"] = headline(run_step("bench.py, parent tree", [sys.executable, "bench.py"] + flags, a.parent_tree, 420))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("(a) permute + planar: %.3f ms (p10 %.3f, p90 %.3f)   (b) px: %.3f ms (p10 %.3f, p90 %.3f)   px_not_slower: %s" % (
        out["permute_path_ms"]["median_ms"], out["permute_path_ms"]["p10_ms"], out["permute_path_ms"]["p90_ms"],
        out["px_path_ms"]["median_ms"], out["px_path_ms"]["p10_ms"], out["px_path_ms"]["p90_ms"], out["px_not_slower"]))
    for k, v in out["profiled_calls"].items():
        print("  %-14s misc %.4f ms" % (k, v["misc_ms"]["median_ms"]))
    print(json.dumps(out.get("bench_py_headline", {})))
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
