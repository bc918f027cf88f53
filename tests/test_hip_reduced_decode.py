"""Reduced-resolution decode on the GPU (run with -m gpu on an MI355X): llicti_decode_images_reduced stops after level r and writes the pixels
whose row and column are multiples of 2^r.  Every comparison is EXACT and the yardstick is the ORIGINAL image, rgb[:, ::s, ::s], which the decode
side never sees; equality with the full decode's subsample is asserted beside it.  Every decode runs on a workspace poisoned with 0xA5 -- the
pixels of the skipped levels are never written, an implementation that reads one finds 0xA5 there -- and once more on a context that has done
nothing else."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_state_dict
from helpers import SWEEP_SHAPES, make_image

pytestmark = pytest.mark.gpu

A_CONTAINERS = ["ac", "rans8", "wrans4", "xrans10", "xrans24", "auto"]
A_SHAPES = [(64, 48), (67, 93), (33, 64), (577, 768), (768, 512)]      # 577: an odd height at every level
B_CONTAINERS = ["ac", "xrans9", "auto"]
B_SHAPES = SWEEP_SHAPES + [(32, 32)]                                  # tests/test_config_b_gpu.py: SHAPES
WEIGHTS = ["rand1337", "trainedlike"]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _new_codec(wname, nlev):
    from llicti_amd.codec import HipCodec
    c = HipCodec("cuda:0")
    if nlev == 2:
        c.set_model(60, 2)
        c.load_state_dict(load_state_dict(f"b_{wname}"))
    else:
        c.load_state_dict(load_state_dict(wname))
    return c


@pytest.fixture(scope="module")
def codecs(torch_mod):
    cache = {}

    def get(wname, nlev=5):
        if (wname, nlev) not in cache:
            cache[(wname, nlev)] = _new_codec(wname, nlev)
        return cache[(wname, nlev)]
    yield get
    for c in cache.values():
        c.close()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _encoder_mode(name, sizes, nlev):
    from llicti_amd.codec import auto_modes, mode_of_name
    if name != "auto":
        return mode_of_name(name)
    modes = auto_modes(sizes, nlev)
    return modes[0] if all(m == modes[0] for m in modes) else modes


def _encode(torch, c, rgbs, name):
    """rgbs: list of [3, H, W] images -> (containers, seg_len, Hs, Ws, the mode(s) the DECODER takes: what the headers say)."""
    Hs, Ws = [r.shape[1] for r in rgbs], [r.shape[2] for r in rgbs]
    mode = _encoder_mode(name, list(zip(Hs, Ws)), c.nlevels)
    if len(set(zip(Hs, Ws))) == 1:
        cont, seg = c.encode(_dev(torch, np.stack(rgbs)), mode=mode if not isinstance(mode, list) else mode[0])
    else:
        cont, seg = c.encode_v(_dev(torch, np.concatenate([r.reshape(-1) for r in rgbs])), Hs, Ws, mode)
    c.check()
    dm = c.container_modes(cont)
    return cont, seg, Hs, Ws, (dm[0] if all(m == dm[0] for m in dm) else dm)


def _reduced_poisoned(c, cont, seg, Hs, Ws, mode, r, rgb_off=None, out=None):
    """llicti_decode_images_reduced on a workspace that holds 0xA5 in every byte; -> list of uint8 [3, Hr, Wr] arrays (host), the flat device result."""
    from llicti_amd.codec import reduced_dims
    c.workspace_v(Hs, Ws, mode)
    c.poison_workspace(0xA5)
    flat = c.decode_reduced(cont, seg, Hs, Ws, mode, r, rgb_off=rgb_off, out=out)
    c.check()
    st = c.image_status(len(Hs))
    assert (st == 0).all(), st
    host = flat.cpu().numpy()
    imgs, pos = [], 0
    for b, (h, w) in enumerate(zip(Hs, Ws)):
        hr, wr = reduced_dims(h, w, r)
        if rgb_off is not None:
            pos = int(rgb_off[b])
        imgs.append(host[pos:pos + 3 * hr * wr].reshape(3, hr, wr))
        pos += 3 * hr * wr
    return imgs, flat


def _matrix(torch, c, make_fresh, rgb, containers, nlev):
    """One image, every container x every r: the reduced decode equals the original's subsample and the full decode's, on the encoding context
    and on a context that has done nothing else."""
    H, W = rgb.shape[1:]
    fresh = make_fresh()
    try:
        for name in containers:
            cont, seg, Hs, Ws, mode = _encode(torch, c, [rgb], name)
            c.workspace(1, H, W, mode)
            c.poison_workspace(0xA5)
            full = c.decode(cont, seg, H, W, mode=mode)
            c.check()
            full = full.cpu().numpy()[0]
            assert np.array_equal(full, rgb), (name, H, W)
            for r in range(nlev + 1):
                s = 1 << r
                want = rgb[:, ::s, ::s]
                for who, ctx in (("same", c), ("fresh", fresh)):
                    got = _reduced_poisoned(ctx, cont, seg, Hs, Ws, mode, r)[0][0]
                    assert got.shape == want.shape, (name, H, W, r, who, got.shape)
                    assert np.array_equal(got, want), (name, H, W, r, who, "differs from the original's subsample")
                    assert np.array_equal(got, full[:, ::s, ::s]), (name, H, W, r, who, "differs from the full decode's subsample")
    finally:
        fresh.close()


@pytest.mark.parametrize("wname", WEIGHTS)
@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("H,W", A_SHAPES)
def test_config_a_every_container_every_r(torch_mod, codecs, H, W, kind, wname):
    rgb = make_image(kind, H, W, 1000 + H + W)
    _matrix(torch_mod, codecs(wname), lambda: _new_codec(wname, 5), rgb, A_CONTAINERS, 5)


@pytest.mark.parametrize("wname", WEIGHTS)
@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("H,W", B_SHAPES)
def test_config_b_every_container_every_r(torch_mod, codecs, H, W, kind, wname):
    rgb = make_image(kind, H, W, 2000 + H + W)
    _matrix(torch_mod, codecs(wname, 2), lambda: _new_codec(wname, 2), rgb, B_CONTAINERS, 2)


def _eval_sizes():
    shapes = [tuple(s) for s in json.load(open(os.path.join(GOLDEN, "eval_shapes.json")))["shapes"]]
    out = []
    for s in shapes:                                   # five different sizes of the reference's test set, in its order
        if s not in out:
            out.append(s)
        if len(out) == 5:
            break
    assert len(out) == 5
    return out


@pytest.mark.parametrize("r", [1, 3])
def test_mixed_sizes_per_image_modes(torch_mod, codecs, r):
    """Five images of different sizes in one call, a mode per image (auto_modes): each image equals its original's subsample and its own B = 1
    reduced decode."""
    torch = torch_mod
    c = codecs("trainedlike")
    sizes = _eval_sizes()
    rgbs = [make_image(("smooth", "noise")[i % 2], h, w, 70 + i) for i, (h, w) in enumerate(sizes)]
    cont, seg, Hs, Ws, modes = _encode(torch, c, rgbs, "auto")
    assert isinstance(modes, list) and len(set(modes)) > 1, "the batch should need per-image modes"
    s = 1 << r
    fresh = _new_codec("trainedlike", 5)
    try:
        for ctx in (c, fresh):
            got = _reduced_poisoned(ctx, cont, seg, Hs, Ws, modes, r)[0]
            for b, rgb in enumerate(rgbs):
                assert np.array_equal(got[b], rgb[:, ::s, ::s]), (b, sizes[b], r)
        for b in range(len(rgbs)):
            solo = _reduced_poisoned(c, cont[b:b + 1].contiguous(), seg[b:b + 1].contiguous(), Hs[b:b + 1], Ws[b:b + 1], modes[b], r)[0][0]
            assert np.array_equal(solo, got[b]), (b, sizes[b], r)
    finally:
        fresh.close()


def test_explicit_output_offsets(torch_mod, codecs):
    """rgb_off: the reduced images at caller-chosen, non-tight, unordered byte offsets; every byte outside them keeps its value."""
    torch = torch_mod
    from llicti_amd.codec import reduced_dims
    c = codecs("rand1337")
    sizes = [(67, 93), (150, 131), (96, 160)]
    rgbs = [make_image("noise", h, w, 5 + i) for i, (h, w) in enumerate(sizes)]
    cont, seg, Hs, Ws, mode = _encode(torch, c, rgbs, "xrans3")
    for r in (1, 2):
        n = [3 * int(np.prod(reduced_dims(h, w, r))) for h, w in sizes]
        off = np.array([n[1] + 50, 7, n[1] + 50 + n[0] + 13], dtype=np.uint64)      # image 1 first, gaps of odd sizes
        total = int(off[2]) + n[2] + 31
        out = torch.full((total,), 0x3C, dtype=torch.uint8, device="cuda:0")
        got, flat = _reduced_poisoned(c, cont, seg, Hs, Ws, mode, r, rgb_off=off, out=out)
        assert flat.data_ptr() == out.data_ptr()
        host = out.cpu().numpy()
        covered = np.zeros(total, dtype=bool)
        for b, rgb in enumerate(rgbs):
            assert np.array_equal(got[b], rgb[:, ::1 << r, ::1 << r]), (b, r)
            covered[int(off[b]):int(off[b]) + n[b]] = True
        assert (host[~covered] == 0x3C).all()
    # the same offsets with the reference-format container (equal sizes): non-tight REDUCED placement does not make the batch "mixed"
    rgbs = [make_image("smooth", 67, 93, 40 + i) for i in range(2)]
    cont, seg, Hs, Ws, mode = _encode(torch, c, rgbs, "ac")
    n = 3 * int(np.prod(reduced_dims(67, 93, 1)))
    off = np.array([n + 9, 0], dtype=np.uint64)
    got, _ = _reduced_poisoned(c, cont, seg, Hs, Ws, mode, 1, rgb_off=off)
    for b, rgb in enumerate(rgbs):
        assert np.array_equal(got[b], rgb[:, ::2, ::2]), b


@pytest.mark.parametrize("nlev,name", [(5, "xrans10"), (5, "ac"), (5, "rans8"), (2, "xrans9"), (2, "ac")])
def test_skipped_levels_are_not_launched(torch_mod, codecs, nlev, name):
    """Under profiling the call reports 3 (nlev - r) band-CNN launches for every r, none at r = nlev; no level below r has CNN time, and a rANS
    decode with r >= 1 spends nothing in the tail kernel."""
    torch = torch_mod
    c = codecs("trainedlike", nlev)
    rgb = make_image("smooth", 150, 131, 9)
    cont, seg, Hs, Ws, mode = _encode(torch, c, [rgb, rgb[:, ::-1].copy()], name)
    c.set_profiling(True)
    try:
        for r in range(nlev + 1):
            got = _reduced_poisoned(c, cont, seg, Hs, Ws, mode, r)[0]
            assert np.array_equal(got[0], rgb[:, ::1 << r, ::1 << r])
            ms, n = c.last_timing()
            assert n == 3 * (nlev - r), (name, r, n)
            cat, per = c.last_timing_detail()
            assert len(per) == 3 * (nlev - r)
            lev = c.last_cnn_level_ms()
            assert all(v == 0 for v in lev[:r]) and all(v > 0 for v in lev[r:nlev]), (r, lev)
            if name != "ac":
                assert (cat["rans_tail"] > 0) == (r == 0), (r, cat)
                assert (cat["rans_stage"] > 0) == (r < nlev), (r, cat)
            else:
                assert (cat["ac"] > 0) == (r < nlev), (r, cat)
    finally:
        c.set_profiling(False)


@pytest.mark.parametrize("name", ["xrans3", "ac", "auto", "rans8", "wrans4"])
def test_r0_is_the_full_decode(torch_mod, codecs, name):
    """reduce = 0 through the new entry point: the bytes, the per-image status words and the launches of decode_v."""
    torch = torch_mod
    c = codecs("trainedlike")
    rgbs = [make_image(k, 150, 131, 3 + i) for i, k in enumerate(("smooth", "noise", "smooth"))]
    cont, seg, Hs, Ws, mode = _encode(torch, c, rgbs, name)
    c.set_profiling(True)
    try:
        c.workspace_v(Hs, Ws, mode)
        c.poison_workspace(0xA5)
        a = c.decode_v(cont, seg, Hs, Ws, mode).clone()
        c.check()
        st_a, n_a = c.image_status(3).copy(), c.last_timing()[1]
        cat_a = c.last_timing_detail()[0]
        builds = c.counter("plan_builds")
        c.poison_workspace(0xA5)
        b = c.decode_reduced(cont, seg, Hs, Ws, mode, 0)
        c.check()
        st_b, n_b = c.image_status(3).copy(), c.last_timing()[1]
        cat_b = c.last_timing_detail()[0]
    finally:
        c.set_profiling(False)
    assert torch.equal(a, b), name
    assert np.array_equal(st_a, st_b) and (st_a == 0).all(), (st_a, st_b)
    assert n_a == n_b == 15 and {k for k, v in cat_a.items() if v > 0} == {k for k, v in cat_b.items() if v > 0}
    assert c.counter("plan_builds") == builds, "reduce = 0 must use the full decode's own plan"
    assert np.array_equal(a.cpu().numpy(), np.concatenate([r.reshape(-1) for r in rgbs]))


@pytest.mark.parametrize("name", ["xrans3", "ac"])
def test_full_decode_after_reduced_on_one_context(torch_mod, codecs, name):
    """Plan-cache interplay: reduced decodes of a batch (tight and explicit placement), then the full decode of the same batch on the same
    context -- byte-identical to the full decode on a context that has done nothing else, with no device synchronisation or allocation on the way
    and the full plan still cached."""
    torch = torch_mod
    c = codecs("rand1337")
    rgbs = [make_image("noise", 96, 160, 30 + i) for i in range(3)]
    cont, seg, Hs, Ws, mode = _encode(torch, c, rgbs, name)
    flat = np.concatenate([r.reshape(-1) for r in rgbs])
    c.workspace_v(Hs, Ws, mode)
    c.poison_workspace(0xA5)
    first = c.decode_v(cont, seg, Hs, Ws, mode).cpu().numpy()              # (the full plan is cached now)
    c.check()
    _reduced_poisoned(c, cont, seg, Hs, Ws, mode, 1)                        # (warm: the reduced plans' blocks exist)
    before = {k: c.counter(k) for k in ("device_syncs", "device_allocs", "plan_builds", "plan_hits")}
    for r in (2, 3, 1, 2):
        got = _reduced_poisoned(c, cont, seg, Hs, Ws, mode, r)[0]
        for b, rgb in enumerate(rgbs):
            assert np.array_equal(got[b], rgb[:, ::1 << r, ::1 << r]), (r, b)
    c.poison_workspace(0xA5)
    again = c.decode_v(cont, seg, Hs, Ws, mode).cpu().numpy()
    c.check()
    assert (c.image_status(3) == 0).all()
    after = {k: c.counter(k) for k in before}
    assert after["plan_builds"] == before["plan_builds"] + 2, (before, after)          # r = 2 and r = 3; r = 1 and the full plan were cached
    assert after["plan_hits"] == before["plan_hits"] + 3, (before, after)
    assert after["device_syncs"] == before["device_syncs"], (before, after)
    fresh = _new_codec("rand1337", 5)
    try:
        fresh.workspace_v(Hs, Ws, mode)
        fresh.poison_workspace(0xA5)
        alone = fresh.decode_v(cont, seg, Hs, Ws, mode).cpu().numpy()
        fresh.check()
    finally:
        fresh.close()
    assert np.array_equal(again, alone) and np.array_equal(again, first) and np.array_equal(again, flat)


def test_reduce_out_of_range_is_einval(torch_mod, codecs):
    torch = torch_mod
    from llicti_amd import _lib
    for nlev, bad in ((5, (6, -1)), (2, (3, -1))):
        c = codecs("rand1337", nlev)
        rgb = make_image("noise", 64, 96, 1)
        cont, seg, Hs, Ws, mode = _encode(torch, c, [rgb], "ac")
        for r in bad:
            with pytest.raises(_lib.LlictiError) as e:
                c.decode_reduced(cont, seg, Hs, Ws, mode, r)
            assert e.value.code == _lib.EINVAL, (nlev, r)
        with pytest.raises(_lib.LlictiError) as e:
            c.decode(cont, seg, 64, 96, mode=mode, reduce=bad[0])
        assert e.value.code == _lib.EINVAL
        got = _reduced_poisoned(c, cont, seg, Hs, Ws, mode, nlev)[0][0]                # the largest r the model has still decodes
        assert np.array_equal(got, rgb[:, ::1 << nlev, ::1 << nlev])


def _as_model_output(torch, sub):
    """What decompres() returns for the uint8 pixels `sub` [3, h, w]: [1, 3, h, w] float32 = u8 / 255, divided on the device as the model does."""
    return (_dev(torch, sub).to(torch.float32) / 255)[None]


@pytest.mark.parametrize("container", ["ac", "auto"])
def test_model_decompres_reduce(torch_mod, container):
    """LLICTI.decompres(bl, dev, reduce=2): [1, 3, Hr, Wr] float32 = u8 / 255 (as the full decode returns) of the original's subsample."""
    torch = torch_mod
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    torch.manual_seed(1337)
    m = LLICTI(default_config(container=container)).to("cuda:0").eval()
    rgb = make_image("smooth", 150, 131, 8)
    x = _dev(torch, rgb.astype(np.float32) / np.float32(255))[None]
    bl, x_ycocg = m.compress(x)
    m.codec().poison_workspace()
    y = m.decompres(bl, torch.device("cuda:0"), reduce=2)
    assert y.dtype == torch.float32 and tuple(y.shape) == (1, 3, 38, 33)
    assert np.array_equal((y[0] * 255).round().to(torch.uint8).cpu().numpy(), rgb[:, ::4, ::4])
    assert torch.equal(y, _as_model_output(torch, rgb[:, ::4, ::4]))
    m.codec().poison_workspace()
    full = m.decompres(bl, torch.device("cuda:0"))
    assert torch.equal(full, _as_model_output(torch, rgb)) and torch.equal(y, full[..., ::4, ::4])


def test_model_decompres_reduce_xorg_and_batches(torch_mod, capsys):
    """xorg is compared at the reduced positions (no error line for the image's own planes, also below the lift kernel's smallest image; an
    error line for others); decompres_batch and decode_batch_async with reduce, equal and mixed sizes."""
    torch = torch_mod
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    torch.manual_seed(1337)
    m = LLICTI(default_config(container="auto")).to("cuda:0").eval()
    sizes = [(150, 131), (96, 160)]          # (two sizes container "auto" codes with the same lane kind: one call decodes one kind)
    rgbs = [make_image("smooth", h, w, 8 + i) for i, (h, w) in enumerate(sizes)]
    xs = [_dev(torch, r.astype(np.float32) / np.float32(255))[None] for r in rgbs]
    bls, ycc = zip(*(m.compress(x) for x in xs))
    capsys.readouterr()
    y = m.decompres(bls[0], torch.device("cuda:0"), xorg=ycc[0], reduce=1)
    assert "Error" not in capsys.readouterr().out
    assert torch.equal(y, _as_model_output(torch, rgbs[0][:, ::2, ::2]))
    m.decompres(bls[0], torch.device("cuda:0"), xorg=ycc[0] + 1.0, reduce=1)      # planes that are not the image's: the check must speak
    assert "Error" in capsys.readouterr().out
    outs = m.decompres_batch(list(bls), torch.device("cuda:0"), reduce=3)          # mixed sizes: a list
    assert isinstance(outs, list)
    for o, r in zip(outs, rgbs):
        assert torch.equal(o, _as_model_output(torch, r[:, ::8, ::8]))
    same = m.decompres_batch([bls[0], bls[0]], torch.device("cuda:0"), reduce=5)  # equal sizes: one tensor
    assert tuple(same.shape) == (2, 3, 5, 5) and torch.equal(same[1:], _as_model_output(torch, rgbs[0][:, ::32, ::32]))
    y = m.decompres(bls[0], torch.device("cuda:0"), xorg=ycc[0], reduce=5)        # 5 x 5 pixels: below the lift kernel's smallest image
    assert "Error" not in capsys.readouterr().out and torch.equal(y, same[:1])
    flat, Hs, Ws = m.decode_batch_async(list(bls), torch.device("cuda:0"), flat=True, reduce=1)
    m.codec().check()
    assert (Hs, Ws) == ([75, 48], [66, 80]) and flat.numel() == 3 * (75 * 66 + 48 * 80)
    assert np.array_equal(flat.cpu().numpy()[:3 * 75 * 66].reshape(3, 75, 66), rgbs[0][:, ::2, ::2])


def test_cli_decode_reduce_roundtrip(torch_mod, tmp_path, capsys):
    """cli encode -> .llic -> cli decode --reduce 1: the written image is the source's [::2, ::2]; the summary names the reduced size; info lists
    the sizes."""
    from llicti_amd import cli, fileio
    rgb = make_image("smooth", 128, 192, 5)
    src, dst, back = tmp_path / "x.ppm", tmp_path / "x.llic", tmp_path / "y.ppm"
    fileio.write_image(str(src), rgb)
    for container in ("ac", "auto"):
        assert cli.main(["encode", str(src), str(dst), "--container", container]) == 0
        capsys.readouterr()
        assert cli.main(["decode", str(dst), str(back), "--reduce", "1"]) == 0
        assert "96x64" in capsys.readouterr().out
        assert np.array_equal(fileio.read_image(str(back)), rgb[:, ::2, ::2])
        assert cli.main(["decode", str(dst), str(back)]) == 0
        assert np.array_equal(fileio.read_image(str(back)), rgb)
    assert cli.main(["info", str(dst)]) == 0
    assert "r=0 192x128, r=1 96x64, r=2 48x32, r=3 24x16, r=4 12x8, r=5 6x4" in capsys.readouterr().out
