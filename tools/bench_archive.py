#!/usr/bin/env python
"""Archives: what do pack_records / unpack_records and the dense copies cost, against today's strided copies and per-image host work?

  python tools/bench_archive.py [--reps 20] [--warmup 3] [--out profiles/archive/bench.json]

Two workloads, container "auto", seed-1337 weights: 24 natural-like images of 768x512 (llicti_amd/synth.py "smooth"), and 8 of 3840x2160 (the
768x512 image tiled: the generator is too slow for 4K).  The batch is encoded once; every variant below starts from its device containers or
from its host bytes, so no encode or band-CNN time is in any figure but the two "decoded" ones, which hold the same decode.
  out    old: the strided D2H copy of B x out_stride bytes + seg_len, then EncodedBatch.lists()'s cut into 49 Python `bytes` per image
         new: pack_records, the offsets to the host, one dense D2H copy of rec_off[B] bytes (what EncodedBatch.records() does)
  in     old: LLICTI._upload_lists (per-image join into a padded, strided pinned buffer, one H2D copy of B x stride bytes)
         new: ArchiveReader.read_batch (one gather into a pinned buffer) + LLICTI._upload_batch (one dense H2D copy, unpack_records)
         each to containers ready on the device ("ready") and through decode_v to pixels ("decoded")
  kernels  pack_records and unpack_records alone between device events, beside a device-to-device hipMemcpyAsync of the same total bytes
One round runs every variant once; `--reps` rounds (at least 5) after `--warmup` untimed ones, in ONE process, so clock and temperature drift
hit all alike; medians and min .. max.  Device figures lie between device events on the compute stream, host legs are wall clock around
calls that end in a synchronise.  The driver itself never touches the GPU: every workload is a child process under its own `timeout`, and the
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
from bench_resized_decode import run_step, stats  # noqa: E402

WORKLOADS = {"natural_24x768x512": (24, 512, 768), "uhd_8x3840x2160": (8, 2160, 3840)}
DECODE_MS = 11.0          # the 24 x 768x512 decode these calls feed (README): the yardstick of "well under 1 %"


def measure(name, reps, warmup):
    import numpy as np
    import torch
    from llicti_amd import archive, fileio
    from llicti_amd.codec import NSEG, container_to_bytestream_list
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
    enc = model.encode_batch_async(imgs)
    lists = enc.lists()
    cont, seg = enc.cont_d, enc.seg_d
    Hs, Ws = [H] * B, [W] * B
    dmode = codec.container_modes(cont)
    dmode = dmode[0] if all(m == dmode[0] for m in dmode) else dmode
    files = [fileio.dumps_llic(bl) for bl in lists]
    total = sum(len(f) for f in files)
    tmp = tempfile.mkdtemp(prefix="llia_bench_")
    path = os.path.join(tmp, "bench.llia")
    blob0, off0 = enc.records()
    records_equal_files = bytes(blob0) == b"".join(files)
    with archive.ArchiveWriter(path, codec.nseg) as aw:
        aw.append_records(blob0, off0)
    reader = archive.ArchiveReader(path)
    cur = torch.cuda.current_stream(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    # ---- out
    stride = cont.shape[1]
    cont_h = torch.empty((B, stride), dtype=torch.uint8, pin_memory=True)
    seg_h = torch.empty((B, NSEG), dtype=torch.int32, pin_memory=True)
    blob_d = torch.empty((total + 4096,), dtype=torch.uint8, device=dev)
    ro_d = torch.empty((B + 1,), dtype=torch.int64, device=dev)
    ro_h = torch.empty((B + 1,), dtype=torch.int64, pin_memory=True)
    rec_h = torch.empty((total + 4096,), dtype=torch.uint8, pin_memory=True)

    def out_old():
        t0 = time.perf_counter()
        ev[0].record()
        seg_h.copy_(seg, non_blocking=True)
        cont_h.copy_(cont, non_blocking=True)
        ev[1].record()
        ev[1].synchronize()
        t1 = time.perf_counter()
        seg_np, cont_np = seg_h.numpy(), cont_h.numpy()
        got = [container_to_bytestream_list(cont_np[b], seg_np[b]) for b in range(B)]
        t2 = time.perf_counter()
        return {"device_ms": ev[0].elapsed_time(ev[1]), "host_cut_ms": (t2 - t1) * 1e3, "wall_ms": (t2 - t0) * 1e3}, got

    def out_new():
        t0 = time.perf_counter()
        ev[0].record()
        codec.pack_records(cont, seg, out=blob_d, rec_off=ro_d)
        ro_h.copy_(ro_d, non_blocking=True)
        cur.synchronize()
        n = int(ro_h[-1])
        rec_h[:n].copy_(blob_d[:n], non_blocking=True)
        ev[1].record()
        ev[1].synchronize()
        t2 = time.perf_counter()
        return {"device_ms": ev[0].elapsed_time(ev[1]), "wall_ms": (t2 - t0) * 1e3}, (rec_h[:n].numpy(), ro_h.numpy())

    # ---- in
    flat_out = torch.empty((sum(3 * h * w for h, w in zip(Hs, Ws)),), dtype=torch.uint8, device=dev)

    def in_old(decode):
        t0 = time.perf_counter()
        _, cont_d, seg_d, _, _, mode, _ = model._upload_lists(lists, dev)
        t1 = time.perf_counter()
        if decode:
            codec.decode_v(cont_d, seg_d, Hs, Ws, mode, out=flat_out)
        cur.synchronize()
        t2 = time.perf_counter()
        return {"host_ms": (t1 - t0) * 1e3, "wall_ms": (t2 - t0) * 1e3}

    def in_new(decode):
        t0 = time.perf_counter()
        batch = reader.read_batch(range(B))
        _, cont_d, seg_d, _, _, mode, _ = model._upload_batch(batch, dev)
        t1 = time.perf_counter()
        if decode:
            codec.decode_v(cont_d, seg_d, Hs, Ws, mode, out=flat_out)
        cur.synchronize()
        t2 = time.perf_counter()
        return {"host_ms": (t1 - t0) * 1e3, "wall_ms": (t2 - t0) * 1e3}

    # ---- kernels alone
    tight = codec.tight_stride(off0, codec.nseg)
    cont_t = torch.empty((B, tight), dtype=torch.uint8, device=dev)
    seg_t = torch.empty((B, NSEG), dtype=torch.int32, device=dev)
    copy_src = torch.empty((total,), dtype=torch.uint8, device=dev)
    copy_dst = torch.empty((total,), dtype=torch.uint8, device=dev)

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    k_pack = lambda: codec.pack_records(cont, seg, out=blob_d, rec_off=ro_d)
    k_unpack = lambda: codec.unpack_records(blob_d[:total], ro_d, out=cont_t, seg_len=seg_t)
    k_copy = lambda: copy_dst.copy_(copy_src, non_blocking=True)

    # ---- correctness of what is timed
    _, got_lists = out_old()
    _, (got_blob, got_off) = out_new()
    codec.check()
    out_ok = got_lists == lists and bytes(got_blob) == b"".join(files) and list(got_off) == list(np.asarray(off0))
    in_old(True)
    want_px = flat_out.clone()
    flat_out.zero_()
    in_new(True)
    codec.check()
    in_ok = bool(torch.equal(flat_out, want_px)) and bool((codec.image_status(B) == 0).all())
    px = np.concatenate([im.reshape(-1) for im in imgs])
    lossless = bool(torch.equal(want_px.cpu(), torch.from_numpy(px)))

    cols = {}

    def add(key, d):
        for k, v in (d.items() if isinstance(d, dict) else [("ms", d)]):
            cols.setdefault(f"{key}.{k}", []).append(v)
    for r in range(warmup + reps):
        row = [("out_old", out_old()[0]), ("out_new", out_new()[0]), ("in_old_ready", in_old(False)), ("in_new_ready", in_new(False)),
               ("in_old_decoded", in_old(True)), ("in_new_decoded", in_new(True)),
               ("kernel_pack", timed(k_pack)), ("kernel_unpack", timed(k_unpack)), ("memcpy_d2d", timed(k_copy))]
        if r >= warmup:
            for key, d in row:
                add(key, d)
    codec.check()
    reader.close()
    os.remove(path)
    os.rmdir(tmp)
    st = {k: stats(v) for k, v in cols.items()}
    med = lambda k: st[k]["median_ms"]
    return {"device": torch.cuda.get_device_name(dev), "images": B, "size": f"{W}x{H}", "container": "auto",
            "record_bytes_total": total, "container_stride": int(stride), "strided_bytes": int(B * stride), "tight_stride": int(tight),
            "strided_over_dense_bytes": round(B * stride / total, 3),
            "ms": st,
            "out_old_over_new_wall": round(med("out_old.wall_ms") / med("out_new.wall_ms"), 3),
            "in_ready_old_over_new_wall": round(med("in_old_ready.wall_ms") / med("in_new_ready.wall_ms"), 3),
            "in_decoded_old_over_new_wall": round(med("in_old_decoded.wall_ms") / med("in_new_decoded.wall_ms"), 3),
            "pack_over_memcpy": round(med("kernel_pack.ms") / med("memcpy_d2d.ms"), 3),
            "unpack_over_memcpy": round(med("kernel_unpack.ms") / med("memcpy_d2d.ms"), 3),
            "pack_plus_unpack_share_of_11ms_decode": round((med("kernel_pack.ms") + med("kernel_unpack.ms")) / DECODE_MS, 5),
            "records_equal_llic_files": bool(records_equal_files and out_ok), "new_path_decodes_the_same_pixels": in_ok, "lossless": lossless}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "archive", "bench.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.reps < 5:
        ap.error("--reps: at least 5 timed repetitions")
    if a.child:
        print(json.dumps(measure(a.child, a.reps, a.warmup)))
        return 0
    out = {"tool": "tools/bench_archive.py", "reps": a.reps, "warmup": a.warmup,
           "metric": "medians over alternating rounds; device_ms / ms between device events on the compute stream, host_ms / wall_ms on the wall clock "
                     "around calls that end in a synchronise; old = strided copies + per-image host work, new = records: pack / unpack on the device + "
                     "one dense copy", "workloads": {}}
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
        print("%-20s %.1f MB of records (strided: %.1f MB)   out: old %.3f ms, new %.3f ms wall   in (ready): old %.3f, new %.3f   in (decoded): old %.3f, new %.3f   "
              "pack %.4f ms, unpack %.4f ms, memcpy %.4f ms (x%.2f, x%.2f)" % (
                  name, w["record_bytes_total"] / 1e6, w["strided_bytes"] / 1e6, m["out_old.wall_ms"]["median_ms"], m["out_new.wall_ms"]["median_ms"],
                  m["in_old_ready.wall_ms"]["median_ms"], m["in_new_ready.wall_ms"]["median_ms"], m["in_old_decoded.wall_ms"]["median_ms"],
                  m["in_new_decoded.wall_ms"]["median_ms"], m["kernel_pack.ms"]["median_ms"], m["kernel_unpack.ms"]["median_ms"],
                  m["memcpy_d2d.ms"]["median_ms"], w["pack_over_memcpy"], w["unpack_over_memcpy"]))
        if not (w["records_equal_llic_files"] and w["new_path_decodes_the_same_pixels"] and w["lossless"]):
            bad.append(name)
    print("wrote", a.out)
    if bad:
        raise SystemExit(f"the new path's bytes or pixels differ on {bad}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
