#!/usr/bin/env python3
"""Known-answer vectors of the progressive record layout (include/llicti_hip.h "PROGRESSIVE RECORDS").

Writes tests/golden/progressive_vectors.npz: per case the container (its segments back to back, and their lengths), the level cuts of every
stream -- the cursors of tests/ref_rans.py's Stream objects behind each level, >> 3 -- and the progressive record tests/ref_progressive.py
makes of the two:
  a_smooth_67x93_x3   config A, the golden case smooth_67x93_tl, 3 xwide streams: the CPU oracle's container
  a_noise_33x40_x64   config A, make_image("noise", 33, 40, 9), seed-1337 weights, 64 xwide streams: two per segment behind length tables,
                      most of them empty (the oracle's container)
  b_noise_40x33_x3    config B, make_image("noise", 40, 33, 9), 3 xwide streams.  The CPU oracle restates config A only, so this container
                      comes from the HIP ENCODER: with an MI355X present it is encoded here, without one its bytes are kept from the file
                      that exists (cuts and record are re-derived from them either way)
The HIP encoder reproduces the oracle's containers byte for byte, so tests/test_hip_progressive.py holds HipCodec.level_cuts and
pack_progressive to these on the device; tests/test_progressive_cpu.py re-derives the file.
Run from the repo root:  python tests/golden/make_progressive_vectors.py [OUT.npz]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_progressive as rp
import ref_rans as rr
from helpers import make_image, padded_to_88
from llicti_amd.weights import pack_state_dict
from oracle import oracle as orc

GOLDEN = os.path.join(ROOT, "tests", "golden")
PATH = os.path.join(GOLDEN, "progressive_vectors.npz")
CASES = {"a_smooth_67x93_x3": ("A", "trainedlike", 3), "a_noise_33x40_x64": ("A", "rand1337", 64), "b_noise_40x33_x3": ("B", "rand1337", 3)}


def image(key):
    if key == "a_smooth_67x93_x3":
        return np.load(os.path.join(GOLDEN, "case_smooth_67x93_tl.npz"))["rgb"]
    return make_image("noise", 33, 40, 9) if key == "a_noise_33x40_x64" else make_image("noise", 40, 33, 9)


def weights(key):
    """the oracle's weights of the case's model (config B: its 60-wide heads zero-padded to the oracle's 88)"""
    model, wname, _ = CASES[key]
    if model == "A":
        return orc.Weights(pack_state_dict(dict(np.load(os.path.join(GOLDEN, f"weights_{wname}.npz")))))
    return orc.Weights(padded_to_88(pack_state_dict(dict(np.load(os.path.join(GOLDEN, f"weights_b_{wname}.npz"))))))


def container(key, old=None):
    """-> the container's segments"""
    model, wname, M = CASES[key]
    if model == "A":
        return rr.segments(orc.encode_image_rans(image(key), weights(key), M, 2))
    import torch
    if torch.cuda.is_available():
        from llicti_amd.codec import HipCodec, MODE_RANS
        c = HipCodec("cuda:0")
        c.set_model(60, 2)
        c.load_state_dict(dict(np.load(os.path.join(GOLDEN, f"weights_b_{wname}.npz"))))
        cont, seg = c.encode(torch.from_numpy(image(key)[None]).cuda(), mode=MODE_RANS(M, wide=2))
        c.check()
        seg_h = seg[0].cpu().numpy()[:22]
        flat = cont[0, :int(seg_h.sum())].cpu().numpy().tobytes()
        c.close()
    else:
        assert old is not None, "config B's container is written by the HIP encoder: run on an MI355X once"
        flat, seg_h = old[f"{key}_bytes"].tobytes(), old[f"{key}_seglen"]
    pos, segs = 0, []
    for ln in seg_h:
        segs.append(flat[pos:pos + int(ln)])
        pos += int(ln)
    return segs


def derive(key, segs):
    """-> (cuts int32 [M][L - 1], the progressive record) of a container; the decode is checked against the image on the way"""
    W = weights(key)
    model = rr.OraclePlanes(segs, W)
    cuts, stages = rp.ref_cuts(segs, model.rows)
    model.place(stages)
    assert np.array_equal(orc.unlift(model.planes), image(key)), key
    return np.array(cuts, np.int32).reshape(len(cuts), -1), rp.to_progressive(rp.plain_record(segs), cuts)


def main(path):
    old = np.load(PATH) if os.path.exists(PATH) else None
    out = {}
    for key in CASES:
        segs = container(key, old)
        cuts, rec = derive(key, segs)
        out[f"{key}_bytes"] = np.frombuffer(b"".join(segs), np.uint8)
        out[f"{key}_seglen"] = np.array([len(s) for s in segs], np.int32)
        out[f"{key}_cuts"] = cuts
        out[f"{key}_record"] = np.frombuffer(rec, np.uint8)
        print(key, "payload", sum(len(s) for s in segs), "record", len(rec), "prefixes", rp.prefixes(rec))
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else PATH)
