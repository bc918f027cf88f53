#!/usr/bin/env python
"""Progressive records: how many bytes does a reduced decode read, and what do the host legs and the two copy kernels cost beside `.llia`'s?

  python tools/bench_progressive.py [--reps 20] [--warmup 3] [--out profiles/progressive/bench.json]

Two workloads, container "auto", seed-1337 weights: 24 natural-like images of 768x512 (llicti_amd/synth.py "smooth"), and 8 of 3840x2160 (the
768x512 image tiled: the generator is too slow for 4K).  The batch is encoded once and written to a `.llia` and a `.llpa` file.
  bytes        P_r / P_0 for r = 0 .. L, summed over the batch
  crops        (4K only) host bytes to resized crops: the boxes of tools/bench_per_image_reduce.py's "uhd" workload (seed 7), each image at its
               own r_b.  new: ProgressiveReader.read_batch(reduce=r_b) + H2D + unpack_progressive + decode_tensor_resized(reduce=r_b);
               old: ArchiveReader.read_batch + H2D + unpack_records + the same decode (the parent's path, unchanged)
  full         all r_b = 0, through decode_v: the progressive path against the plain one, and whether its median lies inside the plain
               path's own min .. max
  kernels      pack_progressive / unpack_progressive (r = 0) and pack_records / unpack_records alone between device events, beside a
               device-to-device copy of the same bytes
  level_cuts   against a full decode_v of the batch
One round runs every leg once; `--reps` rounds (at least 5) after `--warmup` untimed ones, in ONE process, so clock and temperature drift hit
all alike; medians and min .. max.  Device figures lie between device events on the compute stream, host legs are wall clock around calls
that end in a synchronise.  The driver itself never touches the GPU: every workload is a child process under its own `timeout`, and the
first one that fails ends the run.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_resized_decode import MEAN, STD, random_resized_box, run_step, stats  # noqa: E402

WORKLOADS = {"natural_24x768x512": (24, 512, 768), "uhd_8x3840x2160": (8, 2160, 3840)}
SIZE = 224


def measure(name, reps, warmup):
    import numpy as np
    import torch
    from llicti_amd import archive, progressive
    from llicti_amd.codec import NSEG, resized_crop_plan
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    from llicti_amd.synth import make_image
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1337)
    model = LLICTI(default_config(container="auto")).to(dev).eval()
    B, H, W = WORKLOADS[name]
    distinct = 4
    base = [make_image("smooth", 512, 768, 100 + i) for i in range(distinct)]
    if (H, W) != (512, 768):
        base = [np.ascontiguousarray(np.tile(b, (1, -(-H // 512), -(-W // 768)))[:, :H, :W]) for b in base]
    imgs = [base[i % distinct] for i in range(B)]
    codec = model.codec(dev)
    L = codec.nlevels
    enc = model.encode_batch_async(imgs)
    blob0, off0 = enc.records()
    pblob0, poff0, prefix0 = enc.records(progressive=True)
    cont, seg = enc.cont_d, enc.seg_d
    Hs, Ws, sizes = [H] * B, [W] * B, [(H, W)] * B
    dmode = codec.container_modes(cont)
    dmode = dmode[0] if all(m == dmode[0] for m in dmode) else dmode
    same_bytes = all(progressive.to_llic(bytes(pblob0[int(poff0[b]):int(poff0[b + 1])])) == bytes(blob0[int(off0[b]):int(off0[b + 1])]) for b in range(B))
    tmp = tempfile.mkdtemp(prefix="llpa_bench_")
    pa, pp = os.path.join(tmp, "bench.llia"), os.path.join(tmp, "bench.llpa")
    with archive.ArchiveWriter(pa, codec.nseg) as aw:
        aw.append_records(blob0, off0)
    with progressive.ProgressiveWriter(pp, codec.nseg) as pw:
        pw.append_records(pblob0, poff0)
    ar, pr = archive.ArchiveReader(pa), progressive.ProgressiveReader(pp)
    prefix_sum = [int(prefix0[:, r].sum()) for r in range(L + 1)]
    cur = torch.cuda.current_stream(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    # ---- crops (4K): each image at its own r_b
    crops = name.startswith("uhd")
    rng = np.random.default_rng(7)
    full = [random_resized_box(rng, h, w) for h, w in sizes]
    flip = [int(v) for v in rng.integers(0, 2, B)]
    own, boxes = resized_crop_plan(sizes, full, (SIZE, SIZE), per_image=True)
    kw = dict(dtype=torch.float16, mean=MEAN, std=STD)
    out_t = torch.empty((B, 3, SIZE, SIZE), dtype=torch.float16, device=dev)
    flat_out = torch.empty((3 * H * W * B,), dtype=torch.uint8, device=dev)

    def leg(reader, reduce, decode):
        """host bytes -> device containers -> the decode; wall clock, with the host leg's share"""
        t0 = time.perf_counter()
        batch = reader.read_batch(range(B), reduce=reduce) if reader is pr else reader.read_batch(range(B))
        t1 = time.perf_counter()
        _, cont_d, seg_d, _, _, mode, _ = model._upload_batch(batch, dev)
        cur.synchronize()
        t2 = time.perf_counter()
        decode(cont_d, seg_d, mode)
        cur.synchronize()
        t3 = time.perf_counter()
        return {"read_ms": (t1 - t0) * 1e3, "ready_ms": (t2 - t0) * 1e3, "wall_ms": (t3 - t0) * 1e3}, int(batch.blob.numel())

    dec_crops = lambda c_, s_, m_: codec.decode_tensor_resized(c_, s_, Hs, Ws, m_, (SIZE, SIZE), boxes, flip=flip, antialias=True, reduce=own, out=out_t, **kw)
    dec_full = lambda c_, s_, m_: codec.decode_v(c_, s_, Hs, Ws, m_, out=flat_out)

    # ---- kernels alone
    total, ptotal = int(off0[-1]), int(poff0[-1])
    tight = codec.tight_stride(off0, codec.nseg)
    cuts = codec.level_cuts(cont, seg, Hs, Ws, dmode)
    blob_d = torch.empty((total + 4096,), dtype=torch.uint8, device=dev)
    pblob_d = torch.empty((ptotal + 4096,), dtype=torch.uint8, device=dev)
    ro_d, pro_d = (torch.empty((B + 1,), dtype=torch.int64, device=dev) for _ in range(2))
    pre_d = torch.empty((B, 6), dtype=torch.int64, device=dev)
    cont_t = torch.empty((B, tight), dtype=torch.uint8, device=dev)
    seg_t = torch.empty((B, NSEG), dtype=torch.int32, device=dev)
    copy_src, copy_dst = (torch.empty((total,), dtype=torch.uint8, device=dev) for _ in range(2))
    cuts_out = torch.empty_like(cuts)

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    kernels = {
        "kernel_pack_records": lambda: codec.pack_records(cont, seg, out=blob_d, rec_off=ro_d),
        "kernel_unpack_records": lambda: codec.unpack_records(blob_d[:total], ro_d, out=cont_t, seg_len=seg_t),
        "kernel_pack_progressive": lambda: codec.pack_progressive(cont, seg, cuts, out=pblob_d, rec_off=pro_d, prefix=pre_d),
        "kernel_unpack_progressive": lambda: codec.unpack_progressive(pblob_d[:ptotal], pro_d, reduce=0, out=cont_t, seg_len=seg_t),
        "memcpy_d2d": lambda: copy_dst.copy_(copy_src, non_blocking=True),
        "level_cuts": lambda: codec.level_cuts(cont, seg, Hs, Ws, dmode, out=cuts_out),
        "decode_v": lambda: codec.decode_v(cont, seg, Hs, Ws, dmode, out=flat_out),
    }

    # ---- correctness of what is timed
    for fn in kernels.values():
        fn()
    codec.check()
    kernels_ok = bool(torch.equal(cont_t[:, :16], cont[:, :16])) and pblob_d[:ptotal].cpu().numpy().tobytes() == bytes(pblob0) and bool(torch.equal(cuts_out, cuts))
    leg(ar, None, dec_full)
    want_px = flat_out.clone()
    flat_out.zero_()
    leg(pr, 0, dec_full)
    codec.check()
    full_ok = bool(torch.equal(flat_out, want_px)) and bool((codec.image_status(B) == 0).all())
    lossless = bool(torch.equal(want_px.cpu(), torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs]))))
    crops_ok, bytes_old, bytes_new = True, None, None
    if crops:
        _, bytes_old = leg(ar, None, dec_crops)
        want_t = out_t.clone()
        out_t.zero_()
        _, bytes_new = leg(pr, own, dec_crops)
        codec.check()
        crops_ok = bool(torch.equal(out_t, want_t)) and bool((codec.image_status(B) == 0).all())

    cols = {}

    def add(key, d):
        for k, v in (d.items() if isinstance(d, dict) else [("ms", d)]):
            cols.setdefault(f"{key}.{k}", []).append(v)
    for r in range(warmup + reps):
        row = [("full_plain", leg(ar, None, dec_full)[0]), ("full_progressive", leg(pr, 0, dec_full)[0])]
        if crops:
            row += [("crops_plain", leg(ar, None, dec_crops)[0]), ("crops_progressive", leg(pr, own, dec_crops)[0])]
        row += [(k, timed(fn)) for k, fn in kernels.items()]
        if r >= warmup:
            for key, d in row:
                add(key, d)
    codec.check()
    ar.close()
    pr.close()
    os.remove(pa)
    os.remove(pp)
    os.rmdir(tmp)
    st = {k: stats(v) for k, v in cols.items()}
    med = lambda k: st[k]["median_ms"]
    out = {"device": torch.cuda.get_device_name(dev), "images": B, "size": f"{W}x{H}", "container": "auto", "levels": L,
           "record_bytes_total": total, "progressive_record_bytes_total": ptotal,
           "prefix_bytes_total": prefix_sum, "prefix_over_whole": [round(p / prefix_sum[0], 5) for p in prefix_sum],
           "ms": st,
           "full_progressive_over_plain_wall": round(med("full_progressive.wall_ms") / med("full_plain.wall_ms"), 3),
           "full_progressive_median_inside_plain_spread": bool(st["full_plain.wall_ms"]["min_ms"] <= med("full_progressive.wall_ms") <= st["full_plain.wall_ms"]["max_ms"]),
           "pack_progressive_over_memcpy": round(med("kernel_pack_progressive.ms") / med("memcpy_d2d.ms"), 3),
           "unpack_progressive_over_memcpy": round(med("kernel_unpack_progressive.ms") / med("memcpy_d2d.ms"), 3),
           "pack_records_over_memcpy": round(med("kernel_pack_records.ms") / med("memcpy_d2d.ms"), 3),
           "unpack_records_over_memcpy": round(med("kernel_unpack_records.ms") / med("memcpy_d2d.ms"), 3),
           "level_cuts_over_decode_v": round(med("level_cuts.ms") / med("decode_v.ms"), 3),
           "progressive_records_hold_the_llic_bytes": bool(same_bytes), "kernels_ok": kernels_ok, "full_path_decodes_the_same_pixels": full_ok, "lossless": lossless}
    if crops:
        out.update({"crop_size": SIZE, "boxes_full_resolution_yxhw": [list(v) for v in full], "reduces": own,
                    "crops_host_bytes_plain": bytes_old, "crops_host_bytes_progressive": bytes_new,
                    "crops_plain_over_progressive_wall": round(med("crops_plain.wall_ms") / med("crops_progressive.wall_ms"), 3),
                    "crops_plain_over_progressive_ready": round(med("crops_plain.ready_ms") / med("crops_progressive.ready_ms"), 3),
                    "crops_tensor_bit_equal": crops_ok})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "progressive", "bench.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.reps < 5:
        ap.error("--reps: at least 5 timed repetitions")
    if a.child:
        print(json.dumps(measure(a.child, a.reps, a.warmup)))
        return 0
    out = {"tool": "tools/bench_progressive.py", "reps": a.reps, "warmup": a.warmup,
           "metric": "medians over alternating rounds; kernel figures (.ms) between device events on the compute stream; read_ms / ready_ms / wall_ms on the wall "
                     "clock from host bytes (a memory-mapped file in the page cache) to the gathered buffer / to containers ready on the device / through the decode",
           "workloads": {}}
    for name in WORKLOADS:
        out["workloads"][name] = run_step(name, [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps),
                                                 "--warmup", str(a.warmup)], ROOT, 480)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    bad = []
    for name, w in out["workloads"].items():
        m = w["ms"]
        print("%-20s P_r / P_0 = %s   full: plain %.3f ms, progressive %.3f ms wall (inside the plain spread: %s)   pack %.4f / unpack %.4f ms progressive, "
              "%.4f / %.4f ms plain, memcpy %.4f ms   level_cuts %.3f ms, decode_v %.3f ms" % (
                  name, w["prefix_over_whole"], m["full_plain.wall_ms"]["median_ms"], m["full_progressive.wall_ms"]["median_ms"],
                  w["full_progressive_median_inside_plain_spread"], m["kernel_pack_progressive.ms"]["median_ms"], m["kernel_unpack_progressive.ms"]["median_ms"],
                  m["kernel_pack_records.ms"]["median_ms"], m["kernel_unpack_records.ms"]["median_ms"], m["memcpy_d2d.ms"]["median_ms"],
                  m["level_cuts.ms"]["median_ms"], m["decode_v.ms"]["median_ms"]))
        if "reduces" in w:
            print("%-20s crops at r_b = %s: host bytes %d -> %d; ready: plain %.3f ms, progressive %.3f ms; through the decode: plain %.3f ms, progressive %.3f ms" % (
                "", w["reduces"], w["crops_host_bytes_plain"], w["crops_host_bytes_progressive"], m["crops_plain.ready_ms"]["median_ms"],
                m["crops_progressive.ready_ms"]["median_ms"], m["crops_plain.wall_ms"]["median_ms"], m["crops_progressive.wall_ms"]["median_ms"]))
        if not all(w[k] for k in ("progressive_records_hold_the_llic_bytes", "kernels_ok", "full_path_decodes_the_same_pixels", "lossless")) or not w.get("crops_tensor_bit_equal", True):
            bad.append(name)
    print("wrote", a.out)
    if bad:
        raise SystemExit(f"the progressive path's bytes or pixels differ on {bad}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
