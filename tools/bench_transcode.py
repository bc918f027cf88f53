#!/usr/bin/env python
"""Transcode: does one call beat the decode followed by the encode it replaces?

  python tools/bench_transcode.py [--reps 10] [--warmup 3] [--parent-tree /path/to/parent/checkout] [--bench-steps 5]
                                  [--out profiles/transcode/bench.json]

The batch is bench.py's: 24 x 768x512 uniform noise, seed-1337 weights.  Cases (source -> target): xrans64 -> auto, auto -> xrans10, auto -> ac,
ac -> auto.  Both contenders start from the source containers in HBM and end with the target containers there:
  (a) two calls  HipCodec.decode_v into a pixel buffer, then HipCodec.encode_v from it -- all a caller of the parent commit can do;
  (b) transcode  HipCodec.transcode (llicti_transcode_images): one decode's band-CNN launches, a pairs launch per stage, the target's coder.
One round = (a) then (b), timed between device events on the compute stream, every buffer allocated once; `--reps` rounds (at least 5) after
`--warmup` untimed ones, all cases in ONE process.  Medians and the p10 .. p90 spread are reported; (b) launches a strict subset of (a)'s kernels plus
one header kernel, so `transcode_not_slower` asks for (b)'s median <= (a)'s median in every case and states both spreads beside it.  The decode
alone is timed in the same rounds: "close to the decode alone" is the prediction the numbers confirm or correct.  Before anything is timed (b)'s
containers are compared with (a)'s, byte for byte.  One profiled call of each gives the kernel-group ledger (llicti_last_timing_detail).

The driver itself never touches the GPU: every GPU step is a child process under its own `timeout`, and the first step that fails ends the run.
Steps: the measurement above; `bench.py --gpus 1` of this tree; with --parent-tree, `bench.py --gpus 1` of that tree (built there beforehand) --
the headline path launches unchanged code, so the two headlines must agree within their run-to-run spread.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("xrans64", "auto"), ("auto", "xrans10"), ("auto", "ac"), ("ac", "auto")]


def stats(v):
    s = sorted(v)
    n = len(s)

    def pct(p):
        return s[min(n - 1, max(0, int(round(p * (n - 1)))))]
    return {"median_ms": round(statistics.median(s), 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4), "p10_ms": round(pct(0.1), 4),
            "p90_ms": round(pct(0.9), 4), "reps": n}


def measure(reps, warmup):
    """The child's work: (a) against (b), every case, in one process; -> dict."""
    import torch
    import bench
    from llicti_amd.codec import NSEG, HipCodec, auto_modes, mode_of_name, name_of_mode
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1337)
    sd = LLICTI(default_config()).state_dict()
    B, H, W = 24, 512, 768
    rgb = torch.from_numpy(bench.make_batch(B, H, W, 0)).to(dev)
    flat = rgb.contiguous().view(-1)
    c = HipCodec(dev)
    c.load_state_dict(sd)
    Hs, Ws = [H] * B, [W] * B
    stride = c.max_container_bytes(H, W)

    def enc_mode(name):
        return auto_modes([(H, W)])[0] if name == "auto" else mode_of_name(name)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    cases = []
    for src, dst in CASES:
        src_cont, src_seg = c.encode_v(flat, Hs, Ws, enc_mode(src))
        c.check()
        sm = c.container_modes(src_cont)
        src_mode = sm[0] if all(m == sm[0] for m in sm) else sm
        dst_mode = enc_mode(dst)
        rec = torch.empty_like(flat)
        cont_a, seg_a = torch.empty((B, stride), dtype=torch.uint8, device=dev), torch.zeros((B, NSEG), dtype=torch.int32, device=dev)
        cont_b, seg_b = torch.empty_like(cont_a), torch.zeros_like(seg_a)

        def decode_only():
            c.decode_v(src_cont, src_seg, Hs, Ws, src_mode, out=rec)

        def path_a():
            c.decode_v(src_cont, src_seg, Hs, Ws, src_mode, out=rec)
            c.encode_v(rec, Hs, Ws, dst_mode, out=cont_a, seg_len=seg_a)

        def path_b():
            c.transcode(src_cont, src_seg, Hs, Ws, src_mode, dst_mode, out=cont_b, seg_len_out=seg_b)
        # correctness first: the transcode's containers are the two calls', which decode to the batch
        path_a()
        c.poison_workspace()
        path_b()
        c.check()
        assert torch.equal(rec, flat), "the source containers do not decode to the batch"
        assert torch.equal(seg_a, seg_b), f"{src} -> {dst}: segment lengths differ from decode + encode"
        n = seg_a.sum(dim=1)
        assert all(torch.equal(cont_a[b, :int(n[b])], cont_b[b, :int(n[b])]) for b in range(B)), f"{src} -> {dst}: container bytes differ from decode + encode"
        cols = {"two_calls": [], "transcode": [], "decode_alone": []}
        for k in range(warmup + reps):
            t = {"two_calls": timed(path_a), "transcode": timed(path_b), "decode_alone": timed(decode_only)}
            if k >= warmup:
                for key, v in t.items():
                    cols[key].append(v)
        c.check()
        # the kernel groups of one profiled call each
        c.set_profiling(True)
        ledger = {}
        for name, fn in (("decode", decode_only), ("encode", lambda: c.encode_v(rec, Hs, Ws, dst_mode, out=cont_a, seg_len=seg_a)), ("transcode", path_b)):
            fn()
            cat, cnn = c.last_timing_detail()
            ledger[name] = {"groups_ms": {k: round(v, 4) for k, v in cat.items()}, "cnn_launches": len(cnn), "call_ms": round(c.last_timing()[0][0], 4)}
        c.set_profiling(False)
        c.check()
        a, b, d = stats(cols["two_calls"]), stats(cols["transcode"]), stats(cols["decode_alone"])
        tr = ledger["transcode"]
        cases.append({"source": src, "target": dst, "source_container": name_of_mode(src_mode) if isinstance(src_mode, int) else "per image",
                      "target_mode": name_of_mode(dst_mode), "container_bytes": int(n.sum()),
                      "two_calls_ms": a, "transcode_ms": b, "decode_alone_ms": d,
                      "transcode_minus_two_calls_ms": round(b["median_ms"] - a["median_ms"], 4),
                      "transcode_over_decode_alone": round(b["median_ms"] / d["median_ms"], 4),
                      "spread_p10_p90_ms": {"two_calls": round(a["p90_ms"] - a["p10_ms"], 4), "transcode": round(b["p90_ms"] - b["p10_ms"], 4)},
                      "transcode_not_slower": bool(b["median_ms"] <= a["median_ms"]),
                      "pairs_share_of_transcode": round(tr["groups_ms"]["cdf_pairs"] / max(tr["call_ms"], 1e-9), 4),
                      "profiled_calls": ledger})
    c.close()
    return {"device": torch.cuda.get_device_name(dev), "workload": f"{B}x{W}x{H} uniform noise (bench.py's batch), seed-1337 weights, containers in HBM",
            "reps": reps, "warmup": warmup, "metric": "ms per batch between device events, source containers in HBM to target containers in HBM",
            "cases": cases, "transcode_not_slower": all(k["transcode_not_slower"] for k in cases)}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcode", "bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.reps < 5:
        ap.error("--reps: at least 5 timed repetitions")
    if a.child:
        print(json.dumps(measure(a.reps, a.warmup)))
        return 0
    out = {"tool": "tools/bench_transcode.py"}
    out.update(run_step("decode + encode against transcode", [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup", str(a.warmup)],
                        ROOT, 420))
    if a.bench_steps > 0:
        flags = ["--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "2", "--no-cpu-baseline", "--no-extras", "--no-pcie-legs", "--no-ac-leg"]
        out["bench_py_headline"] = {"this_tree": headline(run_step("bench.py, this tree", [sys.executable, "bench.py"] + flags, ROOT, 420))}
        if a.parent_tree:
            out["bench_py_headline"]["parent_tree"] = headline(run_step("bench.py, parent tree", [sys.executable, "bench.py"] + flags, a.parent_tree, 420))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for k in out["cases"]:
        print("%-8s -> %-8s (a) decode + encode %.3f ms (p10 %.3f, p90 %.3f)   (b) transcode %.3f ms (p10 %.3f, p90 %.3f)   decode alone %.3f ms   not slower: %s" % (
            k["source"], k["target"], k["two_calls_ms"]["median_ms"], k["two_calls_ms"]["p10_ms"], k["two_calls_ms"]["p90_ms"],
            k["transcode_ms"]["median_ms"], k["transcode_ms"]["p10_ms"], k["transcode_ms"]["p90_ms"], k["decode_alone_ms"]["median_ms"], k["transcode_not_slower"]))
    print(json.dumps(out.get("bench_py_headline", {})))
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
