#!/usr/bin/env python3
"""Whole archive files, byte for byte, as the writers of llicti_amd/archive.py and llicti_amd/progressive.py wrote them before the two file
layers became one ("Image archives").

Writes tests/golden/archive_files.npz (CPU only):
  llia_a   a `.llia` of config A: the noise_32x32_rand containers of rans_vectors.npz (four stream layouts), the first half through
           append_records from a blob whose offsets do not start at 0, the rest through append_llic; the last name is UTF-8
  llia_b   the same of config B, from rans_b_vectors.npz (an archive holds one model's records, so each model has its file)
  llpa     a `.llpa` of config A: the first two records of progressive_vectors.npz through append_records, the first once more through append
tests/test_archive_files_cpu.py writes the three again with write() below and wants these bytes, and reads them with both readers.
Run from the repo root:  python tests/golden/make_archive_files.py [OUT.npz]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from llicti_amd import archive, fileio, progressive

GOLDEN = os.path.join(ROOT, "tests", "golden")
PATH = os.path.join(GOLDEN, "archive_files.npz")
UTF8_NAME = "bäume/ü.png"
LLPA_KEYS = ["a_smooth_67x93_x3", "a_noise_33x40_x64"]
LLPA_NAMES = ["smooth", "noise64"]


def llic_files(model):
    """name -> the `.llic` bytes of the model's frozen containers (config A: the four of noise_32x32_rand)"""
    vec = np.load(os.path.join(GOLDEN, "rans_vectors.npz" if model == "a" else "rans_b_vectors.npz"))
    out = {}
    for key in sorted(k[:-6] for k in vec.files if k.endswith("_bytes")):
        if model == "a" and not key.startswith("noise_32x32_rand"):
            continue
        flat, pos, segs = vec[key + "_bytes"].tobytes(), 0, []
        for ln in vec[key + "_seglen"]:
            segs.append(flat[pos:pos + int(ln)])
            pos += int(ln)
        # (rans_vectors.npz keeps the 6 x 9 lengths of a bytestream_list, rans_b_vectors.npz the 22 segments)
        out[key] = fileio.dumps_llic([segs[9 * r:9 * r + 9] for r in range(6)] if model == "a" else fileio.segments_to_bytestream_list(segs))
    return out


def names_of(model):
    keys = list(llic_files(model))
    return keys[:-1] + [UTF8_NAME]


def progressive_records():
    vec = np.load(os.path.join(GOLDEN, "progressive_vectors.npz"))
    return [vec[f"{k}_record"].tobytes() for k in LLPA_KEYS]


def write(kind, path):
    """Write the archive `kind` (llia_a, llia_b, llpa) to `path` with the package's writers."""
    if kind == "llpa":
        recs = progressive_records()
        with progressive.ProgressiveWriter(path, 49) as w:
            w.append_records(b"".join(recs), [0, len(recs[0]), len(recs[0]) + len(recs[1])], LLPA_NAMES)
            w.append(recs[0])
        return
    model = kind[-1]
    files, names = list(llic_files(model).values()), names_of(model)
    half = len(files) // 2
    with archive.ArchiveWriter(path, 49 if model == "a" else 22) as aw:
        blob = b"\x00" * 5 + b"".join(files[:half])
        aw.append_records(blob, 5 + np.concatenate(([0], np.cumsum([len(f) for f in files[:half]]))), names[:half])
        for f, nm in zip(files[half:], names[half:]):
            aw.append_llic(f, nm)


KINDS = ("llia_a", "llia_b", "llpa")

if __name__ == "__main__":
    import tempfile
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for kind in KINDS:
            p = os.path.join(d, kind)
            write(kind, p)
            out[kind] = np.frombuffer(open(p, "rb").read(), dtype=np.uint8)
    dst = sys.argv[1] if len(sys.argv) > 1 else PATH
    np.savez_compressed(dst, **out)
    print("wrote", dst, {k: v.size for k, v in out.items()}, os.path.getsize(dst), "bytes")
