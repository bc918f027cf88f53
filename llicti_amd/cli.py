"""python -m llicti_amd.cli encode IN.(png|ppm|jpg) OUT.llic [--container ac|auto|rans<M>|wrans<M>|xrans<M>] [--checkpoint model_best.pth.tar]
                                [--config llicti_B.json] [--digest]
   python -m llicti_amd.cli decode IN.llic OUT.(png|ppm) [--reduce R] [--crc32 HEX] [--checkpoint model_best.pth.tar] [--config llicti_B.json]
   python -m llicti_amd.cli transcode IN.llic OUT.llic [--container ac|auto|rans<M>|wrans<M>|xrans<M>] [--checkpoint model_best.pth.tar] [--config llicti_B.json]
   python -m llicti_amd.cli info   IN.llic | ARCHIVE.llia
   python -m llicti_amd.cli pack   ARCHIVE.llia SRC... [--container ...] [--checkpoint ...] [--config ...] [--batch N] [--digests]
   python -m llicti_amd.cli pack   --progressive ARCHIVE.llpa IMAGE... --container auto|xrans<M> [--checkpoint ...] [--config ...] [--batch N] [--digests]
   python -m llicti_amd.cli unpack ARCHIVE.llia|ARCHIVE.llpa DIR [--as llic|png|ppm] [--checkpoint ...] [--config ...] [--batch N]
   python -m llicti_amd.cli verify ARCHIVE.llia|ARCHIVE.llpa [--batch N] [--checkpoint ...] [--config ...]

File-level front end of the MI355X hot path (needs a GPU: there is no CPU fallback).  Without a checkpoint the
seed-1337 default init is used, as the reference does when `model_best.pth.tar` is missing (agents/base.py:78-80).  --config names the
reference's JSON file the model was trained with (configs/llicti_A.json -- the default -- or llicti_B.json): as the reference's README says,
compress and decompress with the json file that was used to train the model.  decode --reduce R writes the image at 1 / 2^R of its size
(R = 0 .. the model's levels: 5 for config A, 2 for config B; `info` lists the sizes): exactly every 2^R-th pixel of every 2^R-th row, decoded
from the coarse levels alone -- a decimation without smoothing, so fine texture aliases.  transcode rewrites a file in another container
(default "auto") -- the bytes `encode --container ...` gives for the image the file holds -- on the device, at the cost of one decode: no pixels
are made (it needs the model the file was written with, like decode).  pack writes an image archive (llicti_amd/archive.py): SRC are images, coded
in batches of --batch (one encode, one on-device pack of the records and one dense download per batch), or .llic files, taken as they are; unpack
writes every image of an archive into DIR under its name, as the .llic file it holds (no GPU) or decoded to png / ppm (one dense upload, one
on-device unpack and one decode per batch); info on an archive lists its images.  pack --progressive writes a `.llpa` archive of progressive
records (llicti_amd/progressive.py: the same bytes level-major, so that a reduced decode reads a prefix of a record alone; it costs one decode
per batch on top of the encode) -- xwide containers only; info on one prints every image's prefix lengths P_r; unpack --as llic turns its
records back into .llic files on the host.
PIXEL DIGESTS (include/llicti_hip.h: zlib's crc32 of an image's pixels as planar uint8 [3][H][W] bytes, computed on the device): encode --digest
prints the image's as crc32=%08x, decode --crc32 HEX checks the decoded image's against it (exit 1 on a mismatch; not with --reduce); pack
--digests writes ARCHIVE + ".lldg" (llicti_amd/digest.py) beside the archive, whose bytes stay what they are without the flag -- images only,
a .llic file's pixels are not at hand; with --progressive the digests of the decode the pack pays anyway are held against the encode's; info
lists the digests when that manifest is present; verify decodes every image of an archive to an 8x8 tensor -- no image leaves the device --,
compares the decode's digests with the manifest's on the device, prints the names that differ and exits 1 if any does."""
from __future__ import annotations

import argparse
import sys
import time


def _model(container, checkpoint, config_path=None):
    import torch
    from .config import default_config, load_json
    from .graphs.models.LLICTI_nets import LLICTI
    torch.manual_seed(1337)
    cfg = default_config(container=container)
    if config_path:
        cfg.update(load_json(config_path))          # the model's keys of the JSON file; the container stays the command line's
        cfg["container"] = container
    model = LLICTI(cfg).to("cuda:0").eval()
    if checkpoint:
        from .weights import load_reference_state_dict
        load_reference_state_dict(model, torch.load(checkpoint, map_location="cuda:0")["state_dict"])
    return model, torch


def _reduce_arg(v):
    r = int(v)
    if not 0 <= r <= 5:
        raise argparse.ArgumentTypeError("--reduce takes 0 .. 5 (0 .. 2 for a config-B model)")
    return r


def build_parser():
    ap = argparse.ArgumentParser(prog="llicti_amd.cli")
    sub = ap.add_subparsers(dest="cmd", required=True)
    e = sub.add_parser("encode"); e.add_argument("src"); e.add_argument("dst")
    e.add_argument("--container", default="ac"); e.add_argument("--checkpoint", default=None); e.add_argument("--config", default=None)
    e.add_argument("--digest", action="store_true", help="print the image's pixel digest, crc32=%%08x")
    d = sub.add_parser("decode"); d.add_argument("src"); d.add_argument("dst"); d.add_argument("--checkpoint", default=None)
    d.add_argument("--config", default=None)
    d.add_argument("--reduce", type=_reduce_arg, default=0, metavar="R", help="decode at 1 / 2^R of the size (every 2^R-th pixel; no smoothing)")
    d.add_argument("--crc32", type=_crc_arg, default=None, metavar="HEX", help="the pixel digest the decoded image must have (exit 1 otherwise)")
    t = sub.add_parser("transcode"); t.add_argument("src"); t.add_argument("dst")
    t.add_argument("--container", default="auto"); t.add_argument("--checkpoint", default=None); t.add_argument("--config", default=None)
    i = sub.add_parser("info"); i.add_argument("src")
    p = sub.add_parser("pack"); p.add_argument("archive"); p.add_argument("src", nargs="+")
    p.add_argument("--container", default="ac"); p.add_argument("--checkpoint", default=None); p.add_argument("--config", default=None)
    p.add_argument("--batch", type=_batch_arg, default=24, metavar="N", help="images per batched encode")
    p.add_argument("--progressive", action="store_true", help="write a .llpa archive of progressive records (xwide containers: --container auto or xrans<M>)")
    p.add_argument("--digests", action="store_true", help="write the images' pixel digests to ARCHIVE.lldg beside the archive")
    v = sub.add_parser("verify"); v.add_argument("archive")
    v.add_argument("--checkpoint", default=None); v.add_argument("--config", default=None)
    v.add_argument("--batch", type=_batch_arg, default=24, metavar="N", help="images per batched decode")
    u = sub.add_parser("unpack"); u.add_argument("archive"); u.add_argument("dir")
    u.add_argument("--as", dest="fmt", choices=("llic", "png", "ppm"), default="llic")
    u.add_argument("--checkpoint", default=None); u.add_argument("--config", default=None)
    u.add_argument("--batch", type=_batch_arg, default=24, metavar="N", help="images per batched decode")
    return ap


def _batch_arg(v):
    n = int(v)
    if n < 1:
        raise argparse.ArgumentTypeError("--batch takes a positive number of images")
    return n


def _crc_arg(v):
    try:
        n = int(v, 16)
    except ValueError:
        n = -1
    if not 0 <= n <= 0xFFFFFFFF:
        raise argparse.ArgumentTypeError("--crc32 takes up to eight hexadecimal digits")
    return n


def progressive_container_ok(name) -> bool:
    """pack --progressive takes the containers whose streams are xwide: "auto" and "xrans<M>\""""
    return name == "auto" or (name.startswith("xrans") and name[5:].isdigit())


def _groups(keys, limit):
    """Runs of consecutive positions with equal keys, each at most `limit` long -> [(first, end), ...]"""
    out, k = [], 0
    while k < len(keys):
        e = k + 1
        while e < len(keys) and e - k < limit and keys[e] == keys[k]:
            e += 1
        out.append((k, e))
        k = e
    return out


def _info(ar):
    import os
    from .codec import name_of_mode
    from .digest import manifest_path, read_manifest
    from .progressive import ProgressiveReader
    prog = isinstance(ar, ProgressiveReader)
    crcs = read_manifest(manifest_path(ar.path), ar) if os.path.exists(manifest_path(ar.path)) else None
    print(f"{ar.path}: {len(ar)} images, n = {ar.nseg} segments per record, {ar.total_bytes} bytes of {'progressive records' if prog else 'records'}")
    for k in range(len(ar)):
        (H, W), nb = ar.sizes[k], int(ar.offsets[k + 1] - ar.offsets[k])
        tail = "; prefix bytes " + ", ".join(f"P_{r}={int(v)}" for r, v in enumerate(ar.prefix[k])) if prog else ""
        if crcs is not None:
            tail = f", crc32 {crcs[k]:08x}" + tail
        print(f"  {ar.names[k]}: {W}x{H}, container {name_of_mode(ar.modes[k])}, {nb} bytes, {8.0 * nb / (H * W):.4f} bpp{tail}")
    return 0


def _pack(a):
    import os
    from . import fileio
    from .archive import ArchiveWriter
    from .progressive import ProgressiveWriter
    is_llic = [s.lower().endswith(".llic") for s in a.src]
    if a.progressive and not progressive_container_ok(a.container):
        print(f"pack --progressive: container {a.container!r} has no xwide streams; progressive records need --container auto (or xrans<M>)", file=sys.stderr)
        return 2
    if a.progressive and any(is_llic):
        print("pack --progressive takes images: a .llic file's level cuts come from a decode (transcode it, or pack the image)", file=sys.stderr)
        return 2
    if a.digests and any(is_llic):
        print("pack --digests takes images: a .llic file's pixels are not at hand (verify needs the digest of what was encoded)", file=sys.stderr)
        return 2
    names = [os.path.splitext(os.path.basename(s))[0] for s in a.src]
    crcs = []
    model = torch = None
    if not all(is_llic):
        model, torch = _model(a.container, a.checkpoint, a.config)
        nseg = model.codec().nseg
    else:
        with open(a.src[0], "rb") as fh:
            nseg = fh.read(6)[5]
    t0, total = time.time(), 0
    with (ProgressiveWriter if a.progressive else ArchiveWriter)(a.archive, nseg) as aw:
        # a batch is a run of images; the reference format codes one size per call, so its images are read ahead for their sizes
        imgs = {k: fileio.read_image(s, layout="hwc") for k, s in enumerate(a.src) if not is_llic[k]} if a.container == "ac" else {}
        keys = [("llic", k) if is_llic[k] else ("img", imgs[k].shape[:2] if a.container == "ac" else None) for k in range(len(a.src))]
        for g0, g1 in _groups(keys, a.batch):
            if is_llic[g0]:
                with open(a.src[g0], "rb") as fh:
                    data = fh.read()
                aw.append_llic(data, names[g0])
                total += len(data)
                continue
            batch = [imgs[k] if k in imgs else fileio.read_image(a.src[k], layout="hwc") for k in range(g0, g1)]
            enc = model.encode_batch_async(batch, pixels="rgb", digests=a.digests)
            blob, rec_off = enc.records(progressive=a.progressive)[:2]
            if a.digests:
                crcs += enc.digests(verify=a.progressive)      # (a progressive pack has decoded the batch: its digests must be the encode's)
            aw.append_records(blob, rec_off, names[g0:g1])
            total += int(rec_off[-1])
    if a.digests:
        from .digest import archive_index_crc, manifest_path, write_manifest
        write_manifest(manifest_path(a.archive), crcs, archive_index_crc(a.archive))
    print(f"{len(a.src)} images -> {a.archive}: {total} bytes of {'progressive records' if a.progressive else 'records'}, {time.time() - t0:.3f} s")
    return 0


def _unpack(a):
    import os
    from . import fileio
    from .archive import open_archive
    from .progressive import ProgressiveReader, to_llic
    os.makedirs(a.dir, exist_ok=True)
    t0 = time.time()
    with open_archive(a.archive) as ar:
        prog = isinstance(ar, ProgressiveReader)
        names = [os.path.basename(n) or str(k) for k, n in enumerate(ar.names)]
        if a.fmt == "llic":                                  # (on the host: no GPU)
            for k in range(len(ar)):
                with open(os.path.join(a.dir, names[k] + ".llic"), "wb") as fh:
                    fh.write(to_llic(ar.record(k)) if prog else ar.record(k))
        else:
            model, torch = _model("ac", a.checkpoint, a.config)
            # a batch is a run of images; of plain records: of one container kind (the reference format: of one size too)
            keys = [None if prog else (m & ~0xFF, ar.sizes[k] if m == 0 else None) for k, m in enumerate(ar.modes)]
            for g0, g1 in _groups(keys, a.batch):
                outs = model.decode_batch_async(ar.read_batch(range(g0, g1)), torch.device("cuda:0"), pixels="rgb")
                model.codec().check()
                for k, hwc in zip(range(g0, g1), outs):
                    fileio.write_image(os.path.join(a.dir, names[k] + "." + a.fmt), hwc.cpu().numpy(), layout="hwc")
        print(f"{a.archive} -> {a.dir}: {len(ar)} images as {a.fmt}, {time.time() - t0:.3f} s")
    return 0


def _verify(a):
    import os
    from .archive import open_archive
    from .digest import manifest_path, read_manifest
    from .progressive import ProgressiveReader
    t0 = time.time()
    with open_archive(a.archive) as ar:
        if not os.path.exists(manifest_path(a.archive)):
            print(f"{a.archive}: no digest manifest {manifest_path(a.archive)} (pack --digests writes one)", file=sys.stderr)
            return 2
        crcs = read_manifest(manifest_path(a.archive), ar)
        model, torch = _model("ac", a.checkpoint, a.config)
        dev = torch.device("cuda:0")
        want = torch.tensor(crcs, dtype=torch.int64, device=dev)
        prog = isinstance(ar, ProgressiveReader)
        keys = [None if prog else (m & ~0xFF, ar.sizes[k] if m == 0 else None) for k, m in enumerate(ar.modes)]
        bad = []
        for g0, g1 in _groups(keys, a.batch):
            # an 8 x 8 window of every image: the decode is the full one, what leaves it is 192 values per image
            model.decode_batch_async(ar.read_batch(range(g0, g1)), dev, tensor=dict(size=(8, 8), dtype=torch.float16))
            crc, have = model.last_digests()
            differ = ((crc != want[g0:g1]) | (have != 1)).cpu().numpy()
            bad += [g0 + int(k) for k in differ.nonzero()[0]]
        for k in bad:
            print(f"  {ar.names[k]}: the decoded pixels do not have the manifest's crc32 {crcs[k]:08x}")
        print(f"{a.archive}: {len(ar) - len(bad)} of {len(ar)} images verified, {len(bad)} differ, {time.time() - t0:.3f} s")
    return 1 if bad else 0


def main(argv=None):
    a = build_parser().parse_args(argv)
    from . import fileio
    if a.cmd == "pack":
        return _pack(a)
    if a.cmd == "verify":
        return _verify(a)
    if a.cmd == "unpack":
        return _unpack(a)
    if a.cmd == "info":
        from .archive import NotAnArchive, open_archive
        try:
            with open_archive(a.src) as ar:
                return _info(ar)
        except NotAnArchive:
            pass                                             # a .llic file
    if a.cmd == "info":
        from .codec import header_dims, levels_of_header, mode_of_header, name_of_mode, reduced_dims
        bl = fileio.read_llic(a.src)
        H, W = header_dims(bl[0][0] + bl[0][1] + bl[0][2])
        n = sum(len(s) for r in bl for s in r)
        mode = mode_of_header(bl)
        print(f"{a.src}: {W}x{H} RGB, container {name_of_mode(mode)}, {n} bytes, {8.0 * n / (H * W):.4f} bpp")
        sizes = (reduced_dims(H, W, r) for r in range(levels_of_header(bl[0][0][0]) + 1))
        print("decodable sizes (decode --reduce R): " + ", ".join(f"r={r} {w}x{h}" for r, (h, w) in enumerate(sizes)))
        return 0
    if a.cmd == "encode":
        hwc = fileio.read_image(a.src, layout="hwc")         # the file's interleaved rows: uploaded and lifted as they are (no transpose, no float copy)
        model, torch = _model(a.container, a.checkpoint, a.config)
        t0 = time.time()
        enc = model.encode_batch_async([hwc], pixels="rgb", digests=a.digest)
        bl = enc.lists()[0]
        torch.cuda.synchronize()
        dt = time.time() - t0
        fileio.write_llic(a.dst, bl)
        n = sum(len(s) for r in bl for s in r)
        tail = f", crc32={enc.digests()[0]:08x}" if a.digest else ""
        print(f"{a.src} -> {a.dst}: {hwc.shape[1]}x{hwc.shape[0]}, {n} bytes, {8.0 * n / (hwc.shape[0] * hwc.shape[1]):.4f} bpp, {dt:.3f} s{tail}")
        return 0
    if a.cmd == "transcode":
        from .codec import mode_of_header, name_of_mode
        bl = fileio.read_llic(a.src)
        model, torch = _model(a.container, a.checkpoint, a.config)
        t0 = time.time()
        out = model.transcode_batch([bl])[0]
        dt = time.time() - t0
        fileio.write_llic(a.dst, out)
        n0, n = (sum(len(s) for r in x for s in r) for x in (bl, out))
        print(f"{a.src} -> {a.dst}: container {name_of_mode(mode_of_header(bl))} -> {name_of_mode(mode_of_header(out))}, {n0} -> {n} bytes, {dt:.3f} s")
        return 0
    if a.crc32 is not None and a.reduce:
        print("decode --crc32 checks the whole image: it does not go with --reduce", file=sys.stderr)
        return 2
    bl = fileio.read_llic(a.src)
    model, torch = _model("ac", a.checkpoint, a.config)
    t0 = time.time()
    hwc = model.decode_batch_async([bl], torch.device("cuda:0"), reduce=a.reduce, pixels="rgb")[0]      # uint8 [H, W, 3], written so by the decoder
    crc = int(model.last_digests()[0][0]) if a.crc32 is not None else None
    model.codec().check()
    torch.cuda.synchronize()
    dt = time.time() - t0
    fileio.write_image(a.dst, hwc.cpu().numpy(), layout="hwc")
    note = f" (reduce {a.reduce})" if a.reduce else ""
    if crc is not None:
        note += f", crc32={crc:08x}" + ("" if crc == a.crc32 else f" DIFFERS from {a.crc32:08x}")
    print(f"{a.src} -> {a.dst}: {hwc.shape[1]}x{hwc.shape[0]}{note}, {dt:.3f} s")
    return 0 if crc is None or crc == a.crc32 else 1


if __name__ == "__main__":
    sys.exit(main())
