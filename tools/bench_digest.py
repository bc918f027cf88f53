#!/usr/bin/env python
"""Pixel digests: what does llicti_digest_images cost beside a copy of the bytes it reads, and what does verifying a batch cost with it?

  python tools/bench_digest.py [--reps 20] [--warmup 3] [--out profiles/digest/bench.json]

Two workloads, container "auto", seed-1337 weights: 24 natural-like images of 768x512 (llicti_amd/synth.py "smooth") and 8 of 3840x2160 (the
768x512 image tiled).  The batch is encoded once.
  kernel   llicti_digest_images (two kernels) against a device-to-device hipMemcpyAsync of the same 6 H W bytes per image -- the planes it reads
           once; the copy also writes them -- between device events; the ratio of the medians
  verify   new: decode_tensor to an 8 x 8 float16 sink + digests + one device compare against the expected values, ending in the one scalar
           that comes to the host; old (the only way without digests): decode_v, a device-to-host copy of every pixel, zlib.crc32 per image on
           the host.  Wall clock around calls that end in a synchronise
  decode   decode_v with and without a following digests call, between device events; the two swap places every round and follow an untimed
           decode (the host legs in front of them leave the device idle, and the first decode behind that is slower)
One round runs every leg once; `--reps` rounds after `--warmup` untimed ones in ONE process, so clock and temperature drift hit all alike;
medians and min .. max.  The driver never touches the GPU: every workload is a child process under its own `timeout`, and the first one that
fails ends the run.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"natural_24x768x512": (24, 512, 768), "uhd_8x3840x2160": (8, 2160, 3840)}


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "n": len(s)}


def measure(name, reps, warmup):
    import numpy as np
    import torch
    from llicti_amd.codec import _ptr, _stream_ptr, auto_modes
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    from llicti_amd.synth import make_image
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1337)
    model = LLICTI(default_config(container="auto")).to(dev).eval()
    B, H, W = WORKLOADS[name]
    base = [make_image("smooth", 512, 768, 100 + i) for i in range(4)]
    if (H, W) != (512, 768):
        base = [np.ascontiguousarray(np.tile(b, (1, -(-H // 512), -(-W // 768)))[:, :H, :W]) for b in base]
    imgs = [base[i % 4] for i in range(B)]
    src = [zlib.crc32(a.tobytes()) & 0xFFFFFFFF for a in imgs]
    c = model.codec(dev)
    Hs, Ws = [H] * B, [W] * B
    flat = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(dev)
    cont, seg = c.encode_v(flat, Hs, Ws, auto_modes([(H, W)] * B, c.nlevels))
    c.check()
    mode = c.container_modes(cont)
    want = torch.tensor(src, dtype=torch.int64, device=dev)
    hs, ws = np.asarray(Hs, dtype=np.int32), np.asarray(Ws, dtype=np.int32)
    md = np.asarray(mode, dtype=np.int32)
    crc32 = torch.empty((B,), dtype=torch.int32, device=dev)
    have = torch.empty((B,), dtype=torch.int32, device=dev)
    nbytes = 6 * H * W * B
    a_buf = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    b_buf = torch.empty((nbytes,), dtype=torch.uint8, device=dev)

    def raw_digests():
        rc = c.L.llicti_digest_images(c.ctx, B, _ptr(hs), _ptr(ws), _ptr(md), B, None, _ptr(c._ws), c._ws.numel(), _ptr(crc32), _ptr(have), _stream_ptr(dev))
        assert rc == 0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def copy_d2d():
        a_buf.copy_(b_buf, non_blocking=True)      # (contiguous, same dtype, same device: torch issues one hipMemcpyAsync, device to device)

    def verify_new():
        c.decode_tensor(cont, seg, Hs, Ws, mode, (8, 8), dtype=torch.float16)
        crc, hv = c.digests(Hs, Ws, mode)
        assert not bool(((crc != want) | (hv != 1)).any())

    def verify_old():
        host = c.decode_v(cont, seg, Hs, Ws, mode).cpu().numpy()
        n = 3 * H * W
        assert [zlib.crc32(host[b * n:(b + 1) * n].tobytes()) & 0xFFFFFFFF for b in range(B)] == src

    def decode_plain():
        c.decode_v(cont, seg, Hs, Ws, mode)

    def decode_digest():
        c.decode_v(cont, seg, Hs, Ws, mode)
        raw_digests()
    legs = {"digests_ms": lambda: timed(raw_digests), "memcpy_d2d_ms": lambda: timed(copy_d2d), "verify_new_ms": lambda: wall(verify_new),
            "verify_old_ms": lambda: wall(verify_old), "decode_v_ms": lambda: timed(decode_plain), "decode_v_digests_ms": lambda: timed(decode_digest)}
    c.decode_v(cont, seg, Hs, Ws, mode)
    out = {k: [] for k in legs}
    pair = ["decode_v_ms", "decode_v_digests_ms"]
    for r in range(warmup + reps):
        order = [k for k in legs if k not in pair] + (pair if r % 2 == 0 else pair[::-1])      # (the pair swaps places every round ...)
        for k in order:
            if k == order[-2]:
                timed(decode_plain)       # (... behind an untimed decode: the host legs in front of it leave the device idle, and the first decode behind an idle device is slower)
            v = legs[k]()
            if r >= warmup:
                out[k].append(v)
    raw_digests()
    assert (crc32.to(torch.int64) & 0xFFFFFFFF).tolist() == src and have.tolist() == [1] * B
    c.check()
    res = {k: stats(v) for k, v in out.items()}
    res["plane_bytes"] = nbytes
    res["digests_over_memcpy"] = res["digests_ms"]["median"] / res["memcpy_d2d_ms"]["median"]
    res["digests_gb_s"] = nbytes / res["digests_ms"]["median"] / 1e6
    res["verify_old_over_new"] = res["verify_old_ms"]["median"] / res["verify_new_ms"]["median"]
    res["digests_share_of_decode"] = (res["decode_v_digests_ms"]["median"] - res["decode_v_ms"]["median"]) / res["decode_v_ms"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "digest", "bench.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        print("__RESULT__" + json.dumps(measure(a.child, a.reps, a.warmup)))
        return 0
    res = {"what": __doc__.split("\n\n")[0], "reps": a.reps, "warmup": a.warmup, "workloads": {}}
    for name in WORKLOADS:
        p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                           capture_output=True, text=True)
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("__RESULT__")), None)
        if p.returncode != 0 or line is None:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            print(f"{name}: failed with status {p.returncode}; nothing more is started", file=sys.stderr)
            return 1
        res["workloads"][name] = json.loads(line[len("__RESULT__"):])
        print(name, json.dumps(res["workloads"][name]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
