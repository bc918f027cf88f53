"""llicti_transcode_images on the GPU (run with -m gpu on an MI355X): containers of one kind into containers of another at the cost of one decode.
Every check is EXACT.  The yardstick is always the direct encode of the ORIGINAL image -- which the transcode never sees -- in the target mode, one
image per call (an image's container never depends on its batch), and the CPU oracle's container as well on at least one case per target kind.
Every transcode runs on a workspace filled with 0xA5 after the source containers were made, and once more on a context that has done nothing else.
The shapes are the smallest that reach each path: (67, 93) is odd in both directions (pad flags at several levels), (96, 128) a multiple of 32;
(32, 32) / (96, 128) / (192, 256) give the reference-format decoder's chunk pipeline 2 / 4 / 8 chunks at level 0."""

import numpy as np
import pytest

from conftest import load_state_dict
from helpers import make_image

pytestmark = pytest.mark.gpu

POISON = 0xA5
KINDS = ["ac", "rans8", "wrans4", "xrans2", "xrans10"]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def new_codec(wname, tuning=()):
    from llicti_amd.codec import HipCodec
    c = HipCodec("cuda:0")
    if wname.startswith("b_"):
        c.set_model(60, 2)
    c.load_state_dict(load_state_dict(wname))
    for k, v in tuning:
        c.set_tuning(k, v)
    return c


@pytest.fixture(scope="module")
def codecs(torch_mod):
    cache = {}

    def get(wname):
        if wname not in cache:
            cache[wname] = new_codec(wname)
        return cache[wname]
    yield get
    for c in cache.values():
        c.set_tuning("ac_anchor_min_batch", 96)
        c.close()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _mode(name):
    from llicti_amd.codec import mode_of_name
    return mode_of_name(name)


_IMAGES, _DIRECT = {}, {}


def image(H, W, seed):
    """smooth and noise images alternate: cheap and expensive symbols"""
    key = (H, W, seed)
    if key not in _IMAGES:
        _IMAGES[key] = make_image("smooth" if seed % 2 == 0 else "noise", H, W, 900 + seed)
    return _IMAGES[key]


def direct(torch, c, wname, rgb, mode):
    """The yardstick, computed once per (weights, image, mode): the encode of the original image alone -> (container bytes, its 49 segment lengths)"""
    key = (wname, int(mode), rgb.shape, rgb.tobytes())
    if key not in _DIRECT:
        cont, seg = c.encode(_dev(torch, rgb[None]), mode=int(mode))
        c.check()
        seg = seg[0].cpu().numpy().copy()
        _DIRECT[key] = (cont[0, :int(seg.sum())].cpu().numpy().copy(), seg)
    return _DIRECT[key]


def source(torch, c, imgs, mode):
    """device containers of the images in `mode` (one or one per image) -> (containers, seg_len, the modes their headers name)"""
    sizes = [im.shape[1:] for im in imgs]
    flat = _dev(torch, np.concatenate([im.reshape(-1) for im in imgs]))
    cont, seg = c.encode_v(flat, [h for h, _ in sizes], [w for _, w in sizes], mode)
    c.check()
    modes = c.container_modes(cont)
    return cont, seg, (modes[0] if all(m == modes[0] for m in modes) else modes)


def transcode(torch, c, wname, cont, seg, sizes, src_mode, dst_mode, tuning=(), check=True):
    """The transcode on `c` and once more on a fresh context, each on a poisoned workspace and into poisoned outputs -> [(bytes, seg_len row)] per
    image, of the run on `c` (the two runs must agree to the byte).  check=False: the caller reads c's status itself."""
    Hs, Ws = [h for h, _ in sizes], [w for _, w in sizes]
    runs = []
    fresh = new_codec(wname, tuning)
    try:
        for codec in (c, fresh):
            codec.transcode_workspace(Hs, Ws, src_mode, dst_mode)
            codec.poison_workspace(POISON)
            stride = max(codec.max_container_bytes(h, w) for h, w in sizes)
            out = torch.full((len(sizes), stride), POISON, dtype=torch.uint8, device="cuda:0")
            sl = torch.full((len(sizes), 49), -7, dtype=torch.int32, device="cuda:0")
            codec.transcode(cont, seg, Hs, Ws, src_mode, dst_mode, out=out, seg_len_out=sl)
            if check:
                codec.check()
            else:
                torch.cuda.synchronize()
            sl = sl.cpu().numpy()
            runs.append([(out[b, :int(sl[b].sum())].cpu().numpy(), sl[b]) for b in range(len(sizes))])
    finally:
        fresh.close()
    for (g0, s0), (g1, s1) in zip(*runs):
        assert np.array_equal(s0, s1) and np.array_equal(g0, g1), "the fresh context's transcode differs"
    return runs[0]


def assert_same(got, want, what):
    assert np.array_equal(got[1], want[1]), (what, "seg_len differs", got[1][:10], want[1][:10])
    assert np.array_equal(got[0], want[0]), (what, "container bytes differ")


def oracle_list(orc, W_o, rgb, name):
    """the oracle's bytestream_list of an image in container `name` (used as it is)"""
    if name == "ac":
        return orc.encode_image(rgb, W_o)
    if name.startswith("xauto"):
        return orc.encode_image_rans(rgb, W_o, int(name[5:]), wide=2, auto=True)
    wide = {"x": 2, "w": 1, "r": 0}[name[0]]
    return orc.encode_image_rans(rgb, W_o, int(name.lstrip("xwrans")), wide=wide)


# ------------------------------------------------------------------------------------------------ 1. every source x target
@pytest.mark.parametrize("shape", [(67, 93), (96, 128)])
@pytest.mark.parametrize("src", KINDS)
def test_every_source_to_every_target(torch_mod, codecs, oracle_weights, shape, src):
    from llicti_amd.codec import container_to_bytestream_list
    from oracle import oracle as orc
    torch = torch_mod
    wname = "trainedlike" if shape == (67, 93) else "rand1337"
    c = codecs(wname)
    imgs = [image(*shape, 0), image(*shape, 1)]
    cont, seg, src_mode = source(torch, c, imgs, _mode(src))
    assert src_mode == _mode(src)
    seg_h = seg.cpu().numpy()
    for dst in KINDS:
        got = transcode(torch, c, wname, cont, seg, [shape] * 2, src_mode, _mode(dst))
        for b in range(2):
            assert_same(got[b], direct(torch, c, wname, imgs[b], _mode(dst)), (shape, src, dst, b))
            if dst == src:      # ... which is the input itself
                assert np.array_equal(got[b][1], seg_h[b]) and np.array_equal(got[b][0], cont[b, :int(seg_h[b].sum())].cpu().numpy())
        if shape == (67, 93) and src in ("ac", "xrans2"):      # the oracle's container, once per target kind from either family of sources
            assert container_to_bytestream_list(*got[0]) == oracle_list(orc, oracle_weights(wname), imgs[0], dst), (src, dst)


# ------------------------------------------------------------------------------------------------ 2. the reference-format source's chunk pipeline
@pytest.mark.parametrize("anchors", [False, True])
@pytest.mark.parametrize("shape,B", [((32, 32), 2), ((96, 128), 2), ((192, 256), 1)])
def test_reference_format_source_through_its_chunk_pipeline(torch_mod, codecs, shape, B, anchors):
    torch = torch_mod
    wname = "rand1337" if shape == (96, 128) else "trainedlike"
    c = codecs(wname)
    tuning = (("ac_anchor_min_batch", 1 if anchors else 96),)
    imgs = [image(*shape, 10 + b) for b in range(B)]
    cont, seg, src_mode = source(torch, c, imgs, _mode("ac"))
    c.set_tuning(*tuning[0])
    try:
        for dst in ("xrans2", "ac", "rans8"):
            got = transcode(torch, c, wname, cont, seg, [shape] * B, src_mode, _mode(dst), tuning=tuning)
            for b in range(B):
                assert_same(got[b], direct(torch, c, wname, imgs[b], _mode(dst)), (shape, anchors, dst, b))
    finally:
        c.set_tuning("ac_anchor_min_batch", 96)


# ------------------------------------------------------------------------------------------------ 3. mixed sizes, a mode per image
MIXED = [(192, 256), (128, 192), (321, 481)]
NARROW = [(64, 96), (96, 64), (67, 93)]


def X(m):
    from llicti_amd.codec import MODE_RANS
    return MODE_RANS(m, wide=2)


@pytest.mark.parametrize("src", ["fixed", "auto"])
def test_mixed_sizes_with_a_mode_per_image(torch_mod, codecs, oracle_weights, src):
    from llicti_amd.codec import auto_modes, container_to_bytestream_list, name_of_mode
    from oracle import oracle as orc
    torch = torch_mod
    wname = "trainedlike"
    c = codecs(wname)
    auto = auto_modes(MIXED)
    assert [m & 0xFF for m in auto] == [2, 1, 6] and all(m & 0x10000 for m in auto)
    imgs = [image(h, w, 20 + i) for i, (h, w) in enumerate(MIXED)]
    cont, seg, src_mode = source(torch, c, imgs, [X(3), X(1), X(5)] if src == "fixed" else auto)
    if src == "fixed":
        assert src_mode == [X(3), X(1), X(5)]
    for dst in (auto, [X(2), X(4), X(1)], X(3)):
        got = transcode(torch, c, wname, cont, seg, MIXED, src_mode, dst)
        for b in range(3):
            mode_b = dst if isinstance(dst, int) else dst[b]
            assert_same(got[b], direct(torch, c, wname, imgs[b], mode_b), (src, b, hex(mode_b)))
        if dst is auto and src == "fixed":      # the oracle's "auto" container of the smallest image
            assert container_to_bytestream_list(*got[1]) == oracle_list(orc, oracle_weights(wname), imgs[1], name_of_mode(auto[1]))


def test_mixed_sizes_narrow_lanes(torch_mod, codecs):
    from llicti_amd.codec import MODE_RANS
    torch = torch_mod
    wname = "rand1337"
    c = codecs(wname)
    imgs = [image(h, w, 30 + i) for i, (h, w) in enumerate(NARROW)]
    per = [MODE_RANS(2), MODE_RANS(4), MODE_RANS(1)]
    for s, d in ((MODE_RANS(4), per), (per, MODE_RANS(4))):
        cont, seg, src_mode = source(torch, c, imgs, s)
        got = transcode(torch, c, wname, cont, seg, NARROW, src_mode, d)
        for b in range(3):
            assert_same(got[b], direct(torch, c, wname, imgs[b], d if isinstance(d, int) else d[b]), (b,))


# ------------------------------------------------------------------------------------------------ 4. config B
@pytest.mark.parametrize("wname", ["b_rand1337", "b_trainedlike"])
@pytest.mark.parametrize("shape", [(64, 48), (33, 64)])
def test_config_b_both_directions(torch_mod, codecs, shape, wname):
    torch = torch_mod
    c = codecs(wname)
    imgs = [image(*shape, 40), image(*shape, 41)]
    for s, d in (("ac", "xrans9"), ("xrans9", "ac")):
        cont, seg, src_mode = source(torch, c, imgs, _mode(s))
        got = transcode(torch, c, wname, cont, seg, [shape] * 2, src_mode, _mode(d))
        for b in range(2):
            assert_same(got[b], direct(torch, c, wname, imgs[b], _mode(d)), (shape, s, d, b))
            assert int(got[b][1][22:].sum()) == 0      # a 2-level container has 4 + 18 segments


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_launch_nothing(torch_mod):
    from llicti_amd import _lib
    from llicti_amd.codec import MODE_AC, MODE_RANS, MODE_RANS_AUTO, _ptr, _stream_ptr
    torch = torch_mod
    c = new_codec("rand1337")      # a context that has done nothing: a refusal must not even take a plan
    try:
        same, mixed = [(96, 128)] * 3, [(96, 128), (67, 93), (96, 128)]
        stride = c.max_container_bytes(96, 128)
        cont = torch.zeros((3, stride), dtype=torch.uint8, device="cuda:0")
        seg = torch.zeros((3, 49), dtype=torch.int32, device="cuda:0")
        out = torch.zeros((3, stride), dtype=torch.uint8, device="cuda:0")
        seg_out = torch.zeros((3, 49), dtype=torch.int32, device="cuda:0")
        ws = torch.zeros((64 << 20,), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        before = (c.counter("device_syncs"), c.counter("device_allocs"), c.counter("plan_builds"))

        def call(sizes=same, src=X(2), dst=X(2), d_in=cont, in_stride=stride, seg_in=seg, d_ws=ws, ws_bytes=None, d_out=out, out_stride=stride, d_seg=seg_out,
                 Hs=True, Ws=True):
            hs, wsz = np.array([h for h, _ in sizes], dtype=np.int32), np.array([w for _, w in sizes], dtype=np.int32)
            s = np.array([src] if isinstance(src, int) else src, dtype=np.int32)
            d = np.array([dst] if isinstance(dst, int) else dst, dtype=np.int32)
            return c.L.llicti_transcode_images(c.ctx, _ptr(d_in), in_stride, _ptr(seg_in), len(sizes), _ptr(hs) if Hs else None, _ptr(wsz) if Ws else None,
                                               _ptr(s), len(s), _ptr(d), len(d), _ptr(d_ws), ws.numel() if ws_bytes is None else ws_bytes,
                                               _ptr(d_out), out_stride, _ptr(d_seg), _stream_ptr(c.device))

        einval = {
            "auto source": dict(src=MODE_RANS_AUTO(3)),
            "auto source of one image": dict(src=[X(2), MODE_RANS_AUTO(3), X(2)]),
            "mixed lane kinds, source": dict(src=[X(2), MODE_RANS(4), X(2)]),
            "mixed lane kinds, target": dict(dst=[X(2), MODE_RANS(4, wide=1), X(2)]),
            "reference format beside rANS": dict(dst=[MODE_AC, X(2), MODE_AC]),
            "reference-format source, different sizes": dict(sizes=mixed, src=MODE_AC),
            "reference-format target, different sizes": dict(sizes=mixed, dst=MODE_AC),
            "unknown source mode": dict(src=0x777),
            "unknown target mode": dict(dst=0x777),
            "two modes for three images": dict(src=[X(2), X(2)]),
            "null d_in": dict(d_in=None), "null seg_len_in": dict(seg_in=None), "null workspace": dict(d_ws=None), "null d_out": dict(d_out=None),
            "null seg_len_out": dict(d_seg=None), "null Hs": dict(Hs=False), "null Ws": dict(Ws=False),
            "H = 31": dict(sizes=[(31, 128)] * 3), "W = 8161": dict(sizes=[(96, 8161)] * 3),
            "in_stride below the header": dict(in_stride=17 + 3 * 3 * 4 - 1),
            "d_out overlaps d_in": dict(d_out=cont),
        }
        for what, kw in einval.items():
            assert call(**kw) == _lib.EINVAL, what
        nospace = {
            "short workspace": dict(ws_bytes=int(c.L.llicti_workspace_bytes(3, 96, 128, X(2)))),      # enough for either side alone
            "short out_stride": dict(out_stride=17 + 36 + 64),
        }
        for what, kw in nospace.items():
            assert call(**kw) == _lib.ENOSPACE, what
        assert (c.counter("device_syncs"), c.counter("device_allocs"), c.counter("plan_builds")) == before
        c.check()                                  # nothing was launched, nothing is latched
        assert not seg_out.any() and not out.any()
        with pytest.raises(_lib.LlictiError) as e:      # the Python wrapper says so before it sizes a workspace
            c.transcode(cont, seg, [96, 67, 96], [128, 93, 128], MODE_AC, X(2))
        assert e.value.code == _lib.EINVAL
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 6. a bad image among good ones
def test_bad_image_among_good_ones(torch_mod, codecs):
    from llicti_amd._lib import EFORMAT, LlictiError
    torch = torch_mod
    wname = "trainedlike"
    c = codecs(wname)
    shape = (96, 128)
    imgs = [image(*shape, 50 + b) for b in range(3)]
    cont, seg, src_mode = source(torch, c, imgs, X(2))
    cont = cont.clone()
    cont[1, 0] = 0x95                              # the retired v2 tag: a deterministic rejection
    for dst in (X(10), _mode("ac")):
        got = transcode(torch, c, wname, cont, seg, [shape] * 3, X(2), dst, check=False)
        with pytest.raises(LlictiError) as e:
            c.check()
        assert e.value.code == EFORMAT
        assert list(c.image_status(3)) == [0, EFORMAT, 0]
        for b in (0, 2):
            assert_same(got[b], direct(torch, c, wname, imgs[b], dst), (hex(dst), b))
        assert not got[1][1].any() and got[1][1].shape == (49,)      # its row of the segment lengths: 49 zeros
        c.check()                                  # (the status was read and cleared)


# ------------------------------------------------------------------------------------------------ 7. one CNN pass
@pytest.mark.parametrize("src,dst", [("xrans2", "ac"), ("ac", "xrans2")])
def test_one_band_cnn_pass(torch_mod, codecs, src, dst):
    torch = torch_mod
    wname = "rand1337"
    c = codecs(wname)
    shape = (96, 128)
    imgs = [image(*shape, 60), image(*shape, 61)]
    cont, seg, src_mode = source(torch, c, imgs, _mode(src))
    c.set_profiling(True)
    try:
        c.decode(cont, seg, *shape, mode=src_mode)
        c.check()
        dec_cat, dec_cnn = c.last_timing_detail()
        out, sl = c.transcode(cont, seg, [shape[0]] * 2, [shape[1]] * 2, src_mode, _mode(dst))
        c.check()
        cat, cnn = c.last_timing_detail()
    finally:
        c.set_profiling(False)
    assert len(cnn) == len(dec_cnn) > 0            # as many band-CNN launches as the decode alone: one pass
    assert cat["cdf_pairs"] > 0 and dec_cat["cdf_pairs"] == 0
    assert cat["cnn"] > 0 and cat["rans_encode" if dst != "ac" else "ac"] > 0
    sl = sl.cpu().numpy()
    for b in range(2):                             # (profiling changes no byte)
        assert_same((out[b, :int(sl[b].sum())].cpu().numpy(), sl[b]), direct(torch, c, wname, imgs[b], _mode(dst)), (src, dst, b))


# ------------------------------------------------------------------------------------------------ 8. warm path
def test_warm_path_neither_synchronises_nor_allocates(torch_mod, codecs):
    torch = torch_mod
    wname = "rand1337"
    c = codecs(wname)
    shapes = [(96, 128), (67, 93)]
    batches = []
    for k, shape in enumerate(shapes):
        imgs = [image(*shape, 70 + k), image(*shape, 72 + k)]
        cont, seg, src_mode = source(torch, c, imgs, X(2))
        batches.append((shape, imgs, cont, seg, src_mode))

    def run(k):
        shape, imgs, cont, seg, src_mode = batches[k % 2]
        return c.transcode(cont, seg, [shape[0]] * 2, [shape[1]] * 2, src_mode, X(10))
    for k in range(2):
        run(k)
    c.check()
    before = (c.counter("device_syncs"), c.counter("device_allocs"), c.counter("plan_builds"))
    outs = [run(k) for k in range(10)]
    assert (c.counter("device_syncs"), c.counter("device_allocs"), c.counter("plan_builds")) == before
    c.check()
    for k in (8, 9):
        shape, imgs = batches[k % 2][:2]
        sl = outs[k][1].cpu().numpy()
        for b in range(2):
            assert_same((outs[k][0][b, :int(sl[b].sum())].cpu().numpy(), sl[b]), direct(torch, c, wname, imgs[b], X(10)), (k, b))


# ------------------------------------------------------------------------------------------------ 9. Python and CLI
def test_model_transcode_batch(torch_mod):
    from llicti_amd.codec import mode_of_header, name_of_mode
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    torch = torch_mod
    torch.manual_seed(1337)
    model = LLICTI(default_config()).to("cuda:0").eval()          # container "ac": the default
    rgb = image(192, 256, 80)
    x = torch.from_numpy(rgb.astype(np.float32) / np.float32(255)).unsqueeze(0).to("cuda:0")
    bl_ac = model.compress(x)[0]
    got = model.transcode_batch([bl_ac], "auto")
    model.set_container("auto")
    want = model.compress(x)[0]
    assert got == [want] and name_of_mode(mode_of_header(got[0])).startswith("xrans")
    assert model.transcode_batch([bl_ac]) == [want]                # the default target: the model's set_container value
    back = model.decompres(got[0], torch.device("cuda:0"))
    assert np.array_equal((back * 255).round().to(torch.uint8).cpu().numpy()[0], rgb)
    assert model.transcode_batch(got, "ac") == [bl_ac]             # ... and back to the bytes a reader of the reference takes
    # a batch of different sizes, rANS to rANS
    imgs = [image(96, 128, 81), image(67, 93, 82)]
    model.set_container("xrans2")
    lists = model.encode_batch_async(imgs).lists()
    model.set_container("rans4")
    assert model.transcode_batch(lists, "rans4") == model.encode_batch_async(imgs).lists()
    bad = [list(map(list, lists[0])), lists[1]]
    bad[0][0][1] = np.array([0, 100, 0, 255, -100, 0], dtype="<i2").tobytes()      # min Co above max Co: the device refuses the header, codec().check() says so
    from llicti_amd._lib import LlictiError
    with pytest.raises(LlictiError):
        model.transcode_batch(bad, "rans4")


def test_cli_transcode_roundtrip(torch_mod, tmp_path, capsys):
    from llicti_amd import cli, fileio
    rgb = image(192, 256, 90)
    src, a, b, back = (str(tmp_path / n) for n in ("in.ppm", "a.llic", "b.llic", "back.ppm"))
    fileio.write_image(src, rgb)
    assert cli.main(["encode", src, a]) == 0                       # the default container: the reference format
    assert cli.main(["transcode", a, b, "--container", "auto"]) == 0
    capsys.readouterr()
    assert cli.main(["info", a]) == 0
    assert "container ac" in capsys.readouterr().out
    assert cli.main(["info", b]) == 0
    assert "container xrans" in capsys.readouterr().out             # `info` names the new container
    assert cli.main(["decode", b, back]) == 0
    assert open(back, "rb").read() == open(src, "rb").read()
