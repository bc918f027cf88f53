#!/usr/bin/env python3
"""Config B (configs/llicti_B.json: 60-wide heads, 2 levels) on one MI355X: 24 x 768x512 uniform-noise RGB encode + decode in container
"auto", timed like bench.py's step (encode, decode of the containers it wrote, wall clock between synchronisations), one JSON line.

  python tools/bench_config_b.py [--steps K] [--warmup W] [--batch B]

Reports MPix/s and ms per step, bpp and its difference to config B's reference-format container of the same batch, and the band CNN's
fraction of the 157.3 TFLOP/s fp32-MFMA peak: 2 x 111,600 MAC per band-grid position (the three bands' layers, summed) x the positions of
levels 0 and 1, for the encode and the decode, over the CNN launches' event time of one profiled step."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP32_MFMA = 157.3e12
MAC_PER_POS = {0: 240 * 48 + 240 * 60 + 60 * 60, 1: 240 * 72 + 240 * 60 + 60 * 60, 2: 240 * 120 + 240 * 60 + 60 * 60}


def cnn_flops(H, W, levels=2):
    from llicti_amd._lib import level_geom
    f = 0
    for lvl in range(levels):
        for band in range(3):
            _, _, h, w, *_ = level_geom(H, W, lvl, band)
            f += 2 * MAC_PER_POS[band] * h * w
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=24)
    a = ap.parse_args()
    import torch
    from llicti_amd.codec import MODE_AC, auto_modes, name_of_mode
    from llicti_amd.config import CONFIG_B, default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    B, H, W = a.batch, 512, 768
    dev = torch.device("cuda", 0)
    torch.manual_seed(1337)
    model = LLICTI(default_config(**CONFIG_B)).to(dev).eval()
    codec = model.codec(dev)
    rng = np.random.default_rng(0)
    rgb = torch.from_numpy(rng.integers(0, 256, size=(B, 3, H, W), dtype=np.uint8)).to(dev)
    mode = auto_modes([(H, W)], nlevels=2)[0]
    cont, seg = codec.encode(rgb, mode=mode)
    codec.check()
    dm = sorted(set(codec.container_modes(cont)))
    assert len(dm) == 1, dm
    dmode = dm[0]
    codec.poison_workspace()
    rec = codec.decode(cont, seg, H, W, mode=dmode)
    codec.check()
    assert torch.equal(rec, rgb), "decode(encode(x)) != x"

    def step():
        codec.encode(rgb, mode=mode, out=cont, seg_len=seg)
        codec.decode(cont, seg, H, W, mode=dmode, out=rec)
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    codec.check()
    assert torch.equal(rec, rgb)
    nbytes = int(seg.sum().item())
    # the band CNN's event time of one encode and one decode (profiling on: outside the timed steps)
    codec.set_profiling(True)
    codec.encode(rgb, mode=mode, out=cont, seg_len=seg)
    cnn_ms = codec.last_timing()[0][1]
    codec.decode(cont, seg, H, W, mode=dmode, out=rec)
    cnn_ms += codec.last_timing()[0][1]
    codec.set_profiling(False)
    codec.check()
    flops = 2 * B * cnn_flops(H, W)
    ca, sa = codec.encode(rgb, mode=MODE_AC)
    codec.check()
    ac_bytes = int(sa.sum().item())
    mp = B * H * W / 1e6
    print(json.dumps({
        "metric": "config B MPix/s encode+decode", "value": round(mp / dt, 3), "unit": "MPix/s", "ms_per_step": round(dt * 1e3, 3),
        "steps": a.steps, "warmup": a.warmup,
        "workload": f"{B}x{W}x{H} uniform-noise RGB, configs/llicti_B.json shape, seed-1337 weights, container auto",
        "container": name_of_mode(mode), "container_written": name_of_mode(dmode),
        "bpp": round(8.0 * nbytes / (B * H * W), 5), "bpp_delta_vs_ac_container": round(8.0 * (nbytes - ac_bytes) / (B * H * W), 6),
        "cnn_ms_per_step": round(cnn_ms, 3), "cnn_gflop_per_step": round(flops / 1e9, 2),
        "cnn_frac_of_fp32_mfma_peak": round(flops / (cnn_ms * 1e-3) / PEAK_FP32_MFMA, 4),
    }))


if __name__ == "__main__":
    main()
