"""Config B (configs/llicti_B.json: 60-wide heads, 2 levels) on the GPU: the 60-wide band CNN against the float64 restatement of the model
(tests/ref64.py), the reference-format and xwide v4 containers, mixed sizes,
config A and B side by side, the likelihood path and the agent.  Run with -m gpu on an MI355X."""
import logging

import numpy as np
import pytest

import ref64
from conftest import load_case, load_state_dict
from helpers import SWEEP_SHAPES, make_image, tile_edge_classes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _b_config(**over):
    from llicti_amd.config import CONFIG_B, default_config
    c = default_config(**CONFIG_B)
    c.update(over)
    return c


def _b_state_dict(wname):
    """The reference's config-B weights (tests/golden/make_fixtures_config_b.py): seed-1337 init, and the same with make_fixtures.trained_like_."""
    return load_state_dict(f"b_{wname}")


@pytest.fixture(scope="module")
def bcodec(torch_mod):
    from llicti_amd.codec import HipCodec
    cache = {}

    def get(wname):
        if wname not in cache:
            c = HipCodec("cuda:0")
            c.set_model(60, 2)
            c.load_state_dict(_b_state_dict(wname))
            cache[wname] = c
        return cache[wname]
    yield get
    for c in cache.values():
        c.set_tuning("cnn_tile_rows", 0)
        c.set_tuning("force_ragged", 0)
        c.close()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


SHAPES = SWEEP_SHAPES + [(32, 32)]


def test_shapes_cover_tile_edges_at_both_levels():
    """At levels 0 and 1 alone the sweep shapes put tiles into all 72 tile-edge classes."""
    got = set()
    for H, W in SHAPES:
        got |= tile_edge_classes(H, W, levels=(0, 1))
    assert len(got) == 72, len(got)


@pytest.mark.parametrize("wname", ["rand1337", "trainedlike"])
def test_cnn_h60_within_float64_bound(torch_mod, bcodec, wname):
    """Every output of the 60-wide CNN, every band, both levels, every tile form (16 / 8 / 4 rows forced, then automatic), within the rigorous
    fp32 error bound of band_params64."""
    torch = torch_mod
    c = bcodec(wname)
    sd = _b_state_dict(wname)
    for H, W in SHAPES:
        rgb = np.stack([make_image(k, H, W, 11 + H + W) for k in ("smooth", "noise")])
        fpl = c.lift(_dev(torch, rgb))[1]
        fnp = fpl.cpu().numpy()
        for lvl in (0, 1):
            for band in range(3):
                ref = [ref64.band_params64(fnp[i], lvl, band, sd) for i in range(2)]
                bnd = [ref64.cnn_error_bound(fnp[i], lvl, band, sd) for i in range(2)]
                outs = []
                for tr in (16, 8, 4, 0):
                    c.set_tuning("cnn_tile_rows", tr)
                    got = c.params60(c.band_params(fpl, lvl, band)).cpu().numpy().astype(np.float64)
                    for i in range(2):
                        err = np.abs(got[i] - ref[i])
                        assert (err <= bnd[i]).all(), (H, W, lvl, band, tr, float((err - bnd[i]).max()))
                    outs.append(got)
                c.set_tuning("cnn_tile_rows", 0)
                for o in outs[1:]:
                    assert np.array_equal(o, outs[0]), (H, W, lvl, band)      # the tile forms compute the same fmaf chains


def _roundtrip(torch, c, rgb, mode, decode_mode=None):
    B, _, H, W = rgb.shape
    d = _dev(torch, rgb)
    cont, seg = c.encode(d, mode=mode)
    c.check()
    c.poison_workspace()
    rec = c.decode(cont, seg, H, W, mode=decode_mode if decode_mode is not None else (c.container_modes(cont)[0]))
    c.check()
    assert torch.equal(rec, d), (H, W, hex(mode))
    return cont, seg


@pytest.mark.parametrize("H,W", [(32, 32), (67, 93), (96, 160)])
def test_reference_format_container_b(torch_mod, bcodec, H, W):
    """The reference-format container of config B: byte 0 = 2 scales, 22 segments (4 + 18 streams), the raw DC band of level 1, lossless
    on a poisoned workspace; its lists have 3 rows."""
    torch = torch_mod
    from llicti_amd.codec import MODE_AC, container_to_bytestream_list
    c = bcodec("rand1337")
    for kind in ("noise", "smooth"):
        rgb = make_image(kind, H, W, 3)[None]
        cont, seg = _roundtrip(torch, c, rgb, MODE_AC, MODE_AC)
        s = seg.cpu().numpy()[0]
        assert (s[22:] == 0).all() and (s[4:22] > 0).all()
        bl = container_to_bytestream_list(cont[0].cpu().numpy(), s)
        assert len(bl) == 3 and bl[0][0][0] == 2
        h1, w1 = -(-(-(-H // 2)) // 2), -(-(-(-W // 2)) // 2)
        assert bl[0][0][1:] == bytes([h1, w1]) and bl[0][3] == rgb[0][:, ::4, ::4].tobytes()


def test_rans_containers_b(torch_mod, bcodec):
    """xwide v4 in "auto" and with a fixed count: lossless on noise, smooth and odd sizes up to 768x512 and the near-limit 1020x764; at 768x512
    on natural-like content within 0.001 bpp of the reference format."""
    torch = torch_mod
    from llicti_amd.codec import MODE_AC, MODE_RANS, image_mode, mode_of_header
    c = bcodec("rand1337")
    for H, W in ((67, 93), (150, 131), (512, 768), (764, 1020)):
        for kind in ("noise", "smooth"):
            rgb = make_image(kind, H, W, 9)[None]
            m = image_mode(H, W, nlevels=2)
            cont, _ = _roundtrip(torch, c, rgb, m)
            assert cont[0, 0].item() in (0xE9, 2)
            _roundtrip(torch, c, rgb, MODE_RANS(6, wide=2), MODE_RANS(6, wide=2))
    from helpers import make_sampled_image
    for kind in ("noise", "natural"):
        rgb = (make_image("noise", 512, 768, 2) if kind == "noise" else make_sampled_image(512, 768, 4))[None]
        _, seg_r = _roundtrip(torch, c, rgb, image_mode(512, 768, nlevels=2))
        _, seg_a = _roundtrip(torch, c, rgb, MODE_AC, MODE_AC)
        dbpp = 8.0 * (int(seg_r.sum()) - int(seg_a.sum())) / (512 * 768)
        assert dbpp <= 0.001, (kind, dbpp)
    # modes config B does not take, and images too large for its header
    d = _dev(torch, make_image("noise", 64, 64, 1)[None])
    from llicti_amd import _lib
    for mode in (MODE_RANS(4), MODE_RANS(4, wide=1), MODE_RANS(19, wide=2), MODE_RANS(64, wide=2)):
        with pytest.raises(_lib.LlictiError) as e:
            c.encode(d, mode=mode)
        assert e.value.code == _lib.EINVAL
    big = _dev(torch, make_image("noise", 64, 1024, 1)[None])
    with pytest.raises(_lib.LlictiError) as e:
        c.encode(big, mode=MODE_AC)
    assert e.value.code == _lib.EINVAL


def test_mixed_sizes_b_equal_solo(torch_mod, bcodec):
    torch = torch_mod
    from llicti_amd.codec import auto_modes
    c = bcodec("trainedlike")
    sizes = [(96, 160), (67, 93), (150, 131)]
    imgs = [make_image(("noise", "smooth", "noise")[i], h, w, 20 + i) for i, (h, w) in enumerate(sizes)]
    Hs, Ws = [h for h, _ in sizes], [w for _, w in sizes]
    modes = auto_modes(sizes, nlevels=2)
    flat = _dev(torch, np.concatenate([x.reshape(-1) for x in imgs]))
    cont, seg = c.encode_v(flat, Hs, Ws, modes)
    c.check()
    picked = c.container_modes(cont)
    for b, x in enumerate(imgs):
        cs, ss = c.encode(_dev(torch, x[None]), mode=modes[b])
        c.check()
        n = int(ss.sum())
        assert torch.equal(seg[b], ss[0]) and torch.equal(cont[b, :n], cs[0, :n]), b
    c.poison_workspace()
    assert torch.equal(c.decode_v(cont, seg, Hs, Ws, picked), flat)
    c.check()


def test_a_and_b_side_by_side(torch_mod, bcodec):
    """An A context and a B context in one process: A's containers are those of an A-only run; each context refuses the other's containers
    image by image (EFORMAT)."""
    torch = torch_mod
    from llicti_amd import _lib
    from llicti_amd.codec import MODE_AC, MODE_RANS, HipCodec
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    torch.manual_seed(1337)
    sd_a = LLICTI(default_config()).state_dict()
    rgb = _dev(torch, np.stack([make_image("noise", 96, 160, 1), make_image("smooth", 96, 160, 2)]))
    a0 = HipCodec("cuda:0")
    a0.load_state_dict(sd_a)
    ref = {m: [t.clone() for t in a0.encode(rgb, mode=m)] for m in (MODE_AC, MODE_RANS(6, wide=2))}
    a0.check()
    a0.close()
    b = bcodec("rand1337")
    a = HipCodec("cuda:0")
    a.load_state_dict(sd_a)
    for m in (MODE_AC, MODE_RANS(6, wide=2)):
        cb, sb = b.encode(rgb, mode=m)
        b.check()
        ca, sa = a.encode(rgb, mode=m)
        a.check()
        assert torch.equal(sa, ref[m][1])
        for i in range(2):
            n = int(sa[i].sum())
            assert torch.equal(ca[i, :n], ref[m][0][i, :n]), (hex(m), i)
        for ctx, cont, seg in ((a, cb, sb), (b, ca, sa)):
            stride = max(cont.shape[1], ctx.max_container_bytes(96, 160))
            buf = torch.zeros((2, stride), dtype=torch.uint8, device="cuda:0")
            buf[:, :cont.shape[1]] = cont
            ctx.decode(buf, seg, 96, 160, mode=m)
            with pytest.raises(_lib.LlictiError):
                ctx.check()
            assert (ctx.image_status(2) == _lib.EFORMAT).all()
    a.close()


def test_forward_b_two_levels_within_selfinfo64(torch_mod):
    torch = torch_mod
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    torch.manual_seed(1337)
    m = LLICTI(_b_config()).to("cuda:0").eval()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    rgb = make_image("smooth", 64, 96, 4)[None]
    out = m.forward(_dev(torch, rgb))
    assert len(out) == 2 and out[0].shape == (1, 9, 32, 48) and out[1].shape == (1, 9, 16, 24)
    c = m.codec()
    fpl = c.lift_train(_dev(torch, rgb)).cpu().numpy()[0]
    for lvl in (0, 1):
        for band in range(3):
            par = c.params60(c.band_params(_dev(torch, fpl[None]), lvl, band)).cpu().numpy()[0]
            want, tol = ref64.selfinfo64(fpl, lvl, band, par)
            got = out[lvl][0, 3 * band:3 * band + 3].cpu().numpy().astype(np.float64)
            assert (np.abs(got - want) <= tol).all(), (lvl, band)


def test_agent_eval_model_config_b(torch_mod, caplog):
    """LLICTIAgent.eval_model on the model keys of the reference's llicti_B.json (tests/golden/llicti_B_model.json) with mode "eval_model" and
    synthetic test data: every image decodes losslessly and the rate table has 1 + 2 rows."""
    import json
    import os
    from conftest import GOLDEN
    from llicti_amd.agents.llicti_agent import LLICTIAgent
    from llicti_amd.config import default_config
    cfg = default_config()
    cfg.update(json.load(open(os.path.join(GOLDEN, "llicti_B_model.json"))))
    cfg.update(mode="eval_model", test_data="synthetic:48x64x3", gpu_device=0)
    with caplog.at_level(logging.INFO):
        agent = LLICTIAgent(cfg)
        res = agent.run()
    assert len(res) == 3
    assert caplog.text.count("Check: Decoded img matches original") == 3
    table = [r for r in caplog.records if "Test Epoch" in r.getMessage()][-1].getMessage()
    assert table.count("->") == 3


B_CASES = ["b_noise_32x32_rand", "b_noise_67x93_rand", "b_smooth_67x93_tl", "b_smooth_64x48_tl"]


@pytest.mark.parametrize("case", B_CASES)
def test_reference_format_against_oracle_and_reference_fixtures(torch_mod, bcodec, case):
    """Config B's reference-format container, stage by stage, against two independent sources.  The CPU oracle over the kernels' own CNN
    outputs: every table row bit-equal (oracle.cdf_rows), and each of the 18 streams -- at its segment, scale 1 then 0 x band x colour --
    equal to oracle.ac_encode_tables over those rows and the oracle's symbols.  The reference's own code (tests/golden/make_fixtures_config_b.py):
    header segments byte-equal, CNN outputs within 1e-5, symbols exact, table entries within 1 (40 where the sigma floor binds, as for A).
    Then the decode: lossless, and its CNN outputs bit-identical to the encoder's."""
    torch = torch_mod
    from llicti_amd._lib import level_geom
    from llicti_amd.codec import MODE_AC, container_to_bytestream_list
    from oracle import oracle as orc
    z = load_case(case)
    wname = "trainedlike" if case.endswith("_tl") else "rand1337"
    ent_tol = 1 if wname == "trainedlike" else 40
    c = bcodec(wname)
    rgb = z["rgb"]
    _, H, W = rgb.shape
    d = _dev(torch, rgb[None])
    cont, seg = c.encode(d, mode=MODE_AC)
    c.check()
    bl = container_to_bytestream_list(cont[0].cpu().numpy(), seg[0].cpu().numpy())
    assert len(bl) == 3
    assert bl[0][0] == z["hdr0"].tobytes() and bl[0][1] == z["hdr_minmax"].tobytes()
    assert bl[0][2] == z["hdr_pad"].tobytes() and bl[0][3] == z["hdr_dc"].tobytes()
    planes, fpl, mm = c.lift(d)
    p_host, mm_ref = orc.lift(rgb)
    assert np.array_equal(planes[0].cpu().numpy(), p_host)
    enc_par = {}
    for si, lvl in enumerate((1, 0)):
        for band in range(3):
            params = c.band_params(fpl, lvl, band)
            P3 = c.params60(params)[0].cpu().numpy()                               # [h, w, 60]
            enc_par[(lvl, band)] = P3
            ref = z[f"params_s{lvl}_b{band}"]
            got = P3.reshape(-1, 60).T
            if f"paridx_s{lvl}_b{band}" in z:
                got = got[:, z[f"paridx_s{lvl}_b{band}"]]
            else:
                ref = ref.reshape(60, -1)
            assert (np.abs(got - ref) <= 1e-5 * np.maximum(1.0, np.abs(ref))).all(), (case, lvl, band, float(np.abs(got - ref).max()))
            *_, hc, wc = level_geom(H, W, lvl, band)
            a, b = ref64.TARGET[band]
            rows_, cols_ = np.arange(a << lvl, H, 2 << lvl), np.arange(b << lvl, W, 2 << lvl)
            P = P3[:hc, :wc].reshape(-1, 60)
            tg = p_host[:, rows_][:, :, cols_].reshape(3, -1).astype(np.float32) / np.float32(255)
            for clr in range(3):
                minv = -127 if clr == 0 else int(mm_ref[clr])
                maxv = 128 if clr == 0 else int(mm_ref[3 + clr])
                Lp = maxv - minv + 2
                want = orc.cdf_rows(P, clr, tg[0], tg[1], minv, maxv)
                tab = c.cdf_tables(planes, params, mm, lvl, band, clr)[0].cpu().numpy().view(np.uint16)[:, :Lp]
                assert np.array_equal(tab, want), (case, lvl, band, clr)
                clow, chigh, sym = orc.stream_pairs(p_host, mm_ref, lvl, band, clr, P3)
                tag = f"s{lvl}_b{band}_c{clr}"
                assert np.array_equal(sym, z["sym_" + tag].ravel()), tag
                for r, idx in zip(z["cdfrows_" + tag], z["cdfidx_" + tag]):
                    dd = np.abs(tab[idx, :-1].astype(np.int64) - r[:-1].astype(np.int64))
                    assert dd.max() <= ent_tol, (case, tag, int(idx), int(dd.max()))
                stream = orc.ac_encode_tables(want, sym)
                assert stream == orc.ac_encode_pairs(clow, chigh)
                assert bl[1 + si][3 * band + clr] == stream, (case, tag)
    c.poison_workspace()
    rec = c.decode(cont, seg, H, W, mode=MODE_AC)
    c.check()
    assert np.array_equal(rec[0].cpu().numpy(), rgb) and np.array_equal(z["reco_rgb"], rgb)
    # the decoder's CNN outputs (of its last launch: level 0, band x10, read from the workspace of a mixed-size-form call) are the encoder's
    from llicti_amd.codec import MODE_RANS
    mode = MODE_RANS(2, wide=2)
    flat = d.reshape(-1).contiguous()
    ct, sg = c.encode_v(flat, [H], [W], mode)
    c.check()
    p_enc = c.last_params_v([H], [W], mode, 0)
    c.poison_workspace()
    assert torch.equal(c.decode_v(ct, sg, [H], [W], mode), flat)
    c.check()
    p_dec = c.last_params_v([H], [W], mode, 0)
    h0, w0 = enc_par[(0, 2)].shape[:2]
    used = torch.ones(64, dtype=torch.bool, device=p_enc.device)
    used[15::16] = False                                             # (plane 15 of a head is never written)
    assert torch.equal(p_enc[used], p_dec[used])
    got = c.params60(p_dec.view(1, 64, h0, w0))[0].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), enc_par[(0, 2)].view(np.uint32))


@pytest.mark.parametrize("rows", [16, 8, 4])
def test_cnn_h60_mixed_size_forms_equal_solo(torch_mod, bcodec, rows):
    """The six mixed-size (RAGGED) instantiations of the 60-wide CNN: a batch of the sweep's sizes through the tile-list path (force_ragged), each
    image's level-0 band-x10 outputs bit-equal to the equal-size kernel's on that image alone -- which test_cnn_h60_within_float64_bound holds
    against the float64 bound -- and the batch lossless."""
    torch = torch_mod
    from llicti_amd.codec import MODE_RANS
    c = bcodec("trainedlike")
    sizes = SWEEP_SHAPES[::3] + [(32, 32)]
    Hs, Ws = [h for h, _ in sizes], [w for _, w in sizes]
    rgbs = [make_image(("smooth", "noise")[i % 2], h, w, 300 + i) for i, (h, w) in enumerate(sizes)]
    mode = MODE_RANS(2, wide=2)
    try:
        c.set_tuning("cnn_tile_rows", rows)
        c.set_tuning("force_ragged", 1)
        flat = _dev(torch, np.concatenate([r.reshape(-1) for r in rgbs]))
        cont, seg = c.encode_v(flat, Hs, Ws, mode)
        c.check()
        got = [c.last_params_v(Hs, Ws, mode, b) for b in range(len(sizes))]
        c.poison_workspace()
        assert torch.equal(c.decode_v(cont, seg, Hs, Ws, mode), flat)
        c.check()
        c.set_tuning("force_ragged", 0)
        for b, rgb in enumerate(rgbs):
            fpl = c.lift(_dev(torch, rgb[None]))[1]
            solo = c.band_params(fpl, 0, 2)[0].reshape(64, -1)
            used = torch.ones(64, dtype=torch.bool, device=solo.device)
            used[15::16] = False                                     # (plane 15 of a head is never written)
            assert torch.equal(got[b][used], solo[used]), (rows, sizes[b])
    finally:
        c.set_tuning("force_ragged", 0)
        c.set_tuning("cnn_tile_rows", 0)


def test_cli_roundtrip_with_reference_llicti_b_json(torch_mod, tmp_path):
    """python -m llicti_amd.cli encode / decode --config on the reference's llicti_B.json: its model keys (tests/golden/llicti_B_model.json) with the
    file's run keys ("mode": "train", "gpu_device": 1, ...) beside them, and a checkpoint in the reference's format; the decode is lossless."""
    import json
    import os
    from llicti_amd import cli, fileio
    from conftest import GOLDEN
    cfg = json.load(open(os.path.join(GOLDEN, "llicti_B_model.json")))
    cfg.update({"mode": "train", "resume_training": True, "gpu_device": 1, "batch_size": 64, "test_data": "/media/datas/Kodak-images"})
    cpath = tmp_path / "llicti_B.json"
    cpath.write_text(json.dumps(cfg))
    ck = tmp_path / "b.pth"
    torch_mod.save({"state_dict": {k: torch_mod.from_numpy(v) for k, v in _b_state_dict("trainedlike").items()}}, str(ck))
    rgb = make_image("smooth", 128, 192, 5)          # (large enough for one xwide stream in container "auto")
    src, dst, back = tmp_path / "x.ppm", tmp_path / "x.llic", tmp_path / "y.ppm"
    fileio.write_image(str(src), rgb)
    for container in ("ac", "auto"):
        assert cli.main(["encode", str(src), str(dst), "--config", str(cpath), "--checkpoint", str(ck), "--container", container]) == 0
        assert fileio.read_llic(str(dst))[0][0][0] == (2 if container == "ac" else 0xE9)
        assert cli.main(["decode", str(dst), str(back), "--config", str(cpath), "--checkpoint", str(ck)]) == 0
        assert np.array_equal(fileio.read_image(str(back)), rgb)
