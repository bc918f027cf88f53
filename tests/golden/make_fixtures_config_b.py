#!/usr/bin/env python3
"""Generate the config-B golden fixtures under tests/golden/ from the reference's own Python (configs/llicti_B.json: 60-wide heads, 2 levels).

Same method and stand-ins as make_fixtures.py (which this script imports): the reference's hot-path code is imported unmodified, compressai
and torchac are replaced by the in-memory stand-ins documented there, and the torchac stand-in records the (cdf, sym) pair of every stream.
Runs only where the reference is available; only data is written:

  weights_b_{rand1337,trainedlike}.npz        the reference's state_dict of config B (seed 1337; trainedlike = make_fixtures.trained_like_)
  case_b_<name>.npz                          per case: rgb, header segments, CNN params per (level, band) (level 0 of the larger cases: every 5th position), symbols, sampled table rows,
                                             the reconstruction
  llicti_B_model.json                        the model keys of configs/llicti_B.json (settings only), for the CLI test
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_fixtures", os.path.join(OUT, "make_fixtures.py"))
mf = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mf)

MODEL_KEYS = ["ycocg", "clrchs", "clr_joint_mode", "clrjnt0seqmd", "mwsa_joint", "chs", "conv_layers", "combine_layers1toL", "Evens", "Odds",
              "dwtlevels", "useprevlevNN", "wtr_type", "net_type", "lif_prec_bits", "ent_mdl_num", "activfun", "subtract_mean", "distribution",
              "num_mixtures"]


def main():
    recorder = []
    mf._install_standins(recorder)
    sys.path.insert(0, mf.REF)
    from graphs.models.LLICTI_nets import LLICTI  # noqa: E402  (reference-owned code)

    raw = json.load(open(os.path.join(mf.REF, "configs", "llicti_B.json")))
    cfg = mf.Cfg(raw)
    json.dump({k: raw[k] for k in MODEL_KEYS if k in raw}, open(os.path.join(OUT, "llicti_B_model.json"), "w"), indent=1)
    torch.use_deterministic_algorithms(True)
    torch.set_num_threads(4)

    weights = {}
    for wname in ("rand1337", "trainedlike"):
        torch.manual_seed(1337)
        model = LLICTI(cfg).eval()
        if wname == "trainedlike":
            mf.trained_like_(model)
        sd = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
        weights[wname] = model
        np.savez_compressed(os.path.join(OUT, f"weights_b_{wname}.npz"), **sd)
        print(wname, "state_dict keys", len(sd))

    cases = [
        # name, kind, H, W, seed, weights
        ("noise_32x32_rand", "noise", 32, 32, 0, "rand1337"),
        ("noise_67x93_rand", "noise", 67, 93, 1, "rand1337"),
        ("smooth_67x93_tl", "smooth", 67, 93, 3, "trainedlike"),
        ("smooth_64x48_tl", "smooth", 64, 48, 2, "trainedlike"),
    ]
    index = {}
    for name, kind, H, W, seed, wname in cases:
        model = weights[wname]
        rgb = mf.make_image(kind, H, W, seed)
        x = torch.from_numpy(rgb.astype(np.float32) / np.float32(255.0)).unsqueeze(0)
        out = {"rgb": rgb}
        with torch.no_grad():
            params_log = []
            bms = list(model.entropymodel.entmdls_scale_band[0])
            origs = [bm.get_params for bm in bms]

            def mk(orig):
                def f(y):
                    p = orig(y)
                    params_log.append(p.detach().clone().numpy()[0])
                    return p
                return f
            for bm, o in zip(bms, origs):
                bm.get_params = mk(o)
            del recorder[:]
            bl, _ = model.compress(x.clone())
            enc_params = list(params_log)
            enc_rec = list(recorder)
            del params_log[:]
            x_reco = model.decompres(bl, torch.device("cpu"))
            dec_params = list(params_log)
            for bm, o in zip(bms, origs):
                bm.get_params = o
        maxerr = float(((x - x_reco) * 255).abs().max())
        assert maxerr == 0.0, maxerr
        for a, b in zip(enc_params, dec_params):
            assert np.array_equal(a, b)
        assert len(bl) == 3 and all(len(r) == 9 for r in bl)
        assert len(enc_rec) == 18 and len(enc_params) == 6
        out["hdr0"] = np.frombuffer(bl[0][0], dtype=np.uint8)
        out["hdr_minmax"] = np.frombuffer(bl[0][1], dtype=np.int16)
        out["hdr_pad"] = np.frombuffer(bl[0][2], dtype=np.int16)
        out["hdr_dc"] = np.frombuffer(bl[0][3], dtype=np.uint8)
        out["reco_rgb"] = np.rint(x_reco.numpy()[0] * 255).astype(np.uint8)
        k = 0
        for si, scl in enumerate((1, 0)):
            for b in range(3):
                p = enc_params[si * 3 + b]            # 60 x h x w, as get_params returns them (before the mean update)
                if scl == 0 and H * W > 4096:         # (a file stays under 1 MB: every 5th position of level 0 of the larger cases)
                    idx = np.arange(0, p.shape[1] * p.shape[2], 5).astype(np.int32)
                    out[f"paridx_s{scl}_b{b}"] = idx
                    out[f"params_s{scl}_b{b}"] = p.reshape(60, -1)[:, idx]
                else:
                    out[f"params_s{scl}_b{b}"] = p
                for clr in range(3):
                    cdf, sym = enc_rec[k]
                    k += 1
                    cdf = cdf[0, 0].view(np.uint16)
                    sym = sym[0, 0]
                    out[f"sym_s{scl}_b{b}_c{clr}"] = sym
                    hh, ww, Lp = cdf.shape
                    n = hh * ww
                    step = max(1, n // 24)
                    idx = np.arange(0, n, step)[:24]
                    out[f"cdfidx_s{scl}_b{b}_c{clr}"] = idx.astype(np.int32)
                    out[f"cdfrows_s{scl}_b{b}_c{clr}"] = cdf.reshape(n, Lp)[idx]
        np.savez_compressed(os.path.join(OUT, f"case_b_{name}.npz"), **out)
        index[name] = {"kind": kind, "H": H, "W": W, "seed": seed, "weights": wname, "hdr0": [int(v) for v in out["hdr0"]],
                       "pad": int(out["hdr_pad"][0])}
        print(name, index[name], "maxerr", maxerr, "bytes", os.path.getsize(os.path.join(OUT, f"case_b_{name}.npz")))
    json.dump(index, open(os.path.join(OUT, "index_b.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
