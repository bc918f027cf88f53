#!/usr/bin/env python3
"""Frozen config B rANS containers (2 levels, byte 0 = 0xE9, xwide v4 streams), written by the HIP ENCODER: the CPU oracle restates config A
only, so nothing on a machine without a GPU writes config B bytes.  Needs an MI355X.

Writes tests/golden/rans_b_vectors.npz: for one odd and one even shape the container bytes, their segment lengths and SHA-256, and for the odd one the HIP decoders' verdict on a fixed set of single-bit flips; the images come
from tests/helpers.make_image, the weights are the committed config B fixtures.  tests/test_ref_rans.py decodes them with tests/ref_rans.py on the
CPU (CDF rows from the oracle's numerics, the 60-wide heads zero-padded to its 88), tests/test_hip_ref_rans.py holds the HIP encoder to them.
Run from the repo root:  python tests/golden/make_rans_b_vectors.py [OUT.npz]"""
import hashlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from llicti_amd.codec import HipCodec, MODE_RANS
from helpers import B_CORRUPT_BASE, B_VECTORS, corruptions, make_image

GOLDEN = os.path.join(ROOT, "tests", "golden")
out = {}
for key, (kind, H, W, seed, wname, M) in B_VECTORS.items():
    c = HipCodec("cuda:0")
    c.set_model(60, 2)
    c.load_state_dict(dict(np.load(os.path.join(GOLDEN, f"weights_b_{wname}.npz"))))
    x = torch.from_numpy(make_image(kind, H, W, seed)[None]).cuda()
    cont, seg = c.encode(x, mode=MODE_RANS(M, wide=2))
    c.check()
    c.poison_workspace()
    rec = c.decode(cont, seg, H, W, mode=MODE_RANS(M, wide=2))
    c.check()
    assert torch.equal(rec, x), key
    seg_h = seg[0].cpu().numpy()
    flat = cont[0, :int(seg_h.sum())].cpu().numpy().tobytes()
    assert flat[0] == 0xE9 and (seg_h[22:] == 0).all()
    out[f"{key}_bytes"] = np.frombuffer(flat, np.uint8)
    out[f"{key}_seglen"] = seg_h[:22].astype(np.int32)
    out[f"{key}_sha256"] = np.frombuffer(hashlib.sha256(flat).digest(), np.uint8)
    print(key, len(flat), hashlib.sha256(flat).hexdigest()[:16])
    if key == B_CORRUPT_BASE:
        # the HIP decoders' verdict on the fixed set of single-bit flips of stream 0 (helpers.corruptions, seed 11), next to an untouched neighbour
        # on a poisoned workspace: status != 0, or the SHA-256 of the pixels it decoded to -- what tests/test_ref_rans.py holds ref_rans to on the CPU
        from llicti_amd._lib import EFORMAT, LlictiError
        cont2, seg2 = c.encode(torch.cat([x, x]), mode=MODE_RANS(M, wide=2))
        c.check()
        off = int(seg_h[:4].sum())
        flips = corruptions(flat[off:off + int(seg_h[4])], 256, "v4", seed=11)
        status, digests = [], []
        for _, bit in flips:
            bad = cont2.clone()
            bad[1, off + (bit >> 3)] ^= 1 << (bit & 7)
            c.workspace(2, H, W, MODE_RANS(M, wide=2))
            c.poison_workspace(0xA5)
            rec = c.decode(bad, seg2, H, W, mode=MODE_RANS(M, wide=2))
            try:
                c.check()
            except LlictiError as e:
                assert e.code == EFORMAT, e
            st = c.image_status(2)
            assert st[0] == 0 and torch.equal(rec[0], x[0])
            status.append(int(st[1] != 0))
            digests.append(np.frombuffer(hashlib.sha256(rec[1].cpu().numpy().tobytes()).digest(), np.uint8))
        out[f"{key}_flip_bits"] = np.array([b for _, b in flips], np.int32)
        out[f"{key}_flip_refused"] = np.array(status, np.uint8)
        out[f"{key}_flip_sha256"] = np.stack(digests)
        print(key, "flips", len(flips), "refused", int(sum(status)))
    c.close()
np.savez_compressed(sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLDEN, "rans_b_vectors.npz"), **out)
