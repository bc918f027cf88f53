"""Tensor options on the GPU (run with -m gpu on an MI355X): the channels-last layout of the three tensor decodes and windows padded past their
image (llicti_decode_images_tensor_o and kin; HipCodec.decode_tensor(channels_last=, pad=), decode_tensor_resized / decode_tensor_views
(channels_last=)).  Every check is EXACT.  The images are the test's own inputs and the codec is lossless, so every expected tensor is built on
the CPU from the ORIGINAL pixels: tests/ref_pad.py (the header's index map, restated) -> flip -> ref_resize.finish (the header's arithmetic), or
ref_resize.resized_crop for boxes -- never from another call of the library, except where a case says (identity).  The sizes are those the
sibling tests run: 67x93 (W % 4 != 0), 64x96 (4-element loads and stores), and the mixed batch 150x131 + 96x160."""
import numpy as np
import pytest

import ref_pad
import ref_resize as rr
from conftest import load_state_dict
from helpers import StreamGate, make_image

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MIXED = [(150, 131), (96, 160)]
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
AWKWARD = ((0.1, 0.3337, 0.9), (0.007, 1.0, 3.3))
PAD_MODES = ("constant", "edge", "reflect", "symmetric")
POISON = 0xA5


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def codecs(torch_mod):
    from llicti_amd.codec import HipCodec
    cache = {}

    def get(nlev=5):
        if nlev not in cache:
            c = HipCodec(DEV)
            if nlev == 2:
                c.set_model(60, 2)
                c.load_state_dict(load_state_dict("b_trainedlike"))
            else:
                c.load_state_dict(load_state_dict("trainedlike"))
            cache[nlev] = c
        return cache[nlev]
    yield get
    for c in cache.values():
        c.close()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Batch:
    """One encoded batch, made once per (model, container, sizes, seed): the ORIGINAL pixels (the yardstick of every test here), the containers
    on the device and the mode a decoder takes for them."""

    def __init__(self, torch, c, nlev, name, sizes, seed):
        from llicti_amd.codec import auto_modes, mode_of_name
        self.sizes = list(sizes)
        self.Hs, self.Ws = [h for h, _ in sizes], [w for _, w in sizes]
        self.rgbs = [make_image(("smooth", "noise")[i % 2], h, w, seed + i) for i, (h, w) in enumerate(sizes)]
        if name == "auto":
            m = auto_modes(self.sizes, nlev)
            enc = m[0] if all(v == m[0] for v in m) else m
        else:
            enc = mode_of_name(name)
        if len(set(self.sizes)) == 1:
            self.cont, self.seg = c.encode(_dev(torch, np.stack(self.rgbs)), mode=enc if isinstance(enc, int) else enc[0])
        else:
            self.cont, self.seg = c.encode_v(_dev(torch, np.concatenate([r.reshape(-1) for r in self.rgbs])), self.Hs, self.Ws, enc)
        c.check()
        modes = c.container_modes(self.cont)
        self.mode = modes[0] if all(m == modes[0] for m in modes) else modes


_BATCHES = {}


def batch(torch, c, nlev, name, sizes, seed=700):
    key = (nlev, name, tuple(sizes), seed)
    if key not in _BATCHES:
        _BATCHES[key] = Batch(torch, c, nlev, name, sizes, seed)
    return _BATCHES[key]


def tname(torch, dt):
    return {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}[dt]


def rounded(torch, v, dt):
    """the float32 value of float v rounded to dtype dt"""
    return float(torch.tensor(np.float32(v)).to(dt).float())


def expect(torch, bt, size, origin=None, flip=None, reduce=0, mode=None, fill=(0, 0, 0), space="pixel", mean=None, std=None, dtype=None):
    """The CPU tensor of a window call, float32 values [B, 3, Ho, Wo], from the ORIGINAL pixels: image b decimated by its reduce, its window
    through ref_pad (mode None: no padding, the window lies inside), ref_resize.finish, the fill elements of space "output", the flip."""
    dtype = torch.float32 if dtype is None else dtype
    B = len(bt.sizes)
    rs = [reduce] * B if isinstance(reduce, int) else list(reduce)
    fill3 = [float(fill)] * 3 if isinstance(fill, (int, float)) else [float(v) for v in fill]
    out = []
    for b in range(B):
        img = bt.rgbs[b][:, ::1 << rs[b], ::1 << rs[b]]
        y0, x0 = (0, 0) if origin is None else (int(origin[0][b]), int(origin[1][b]))
        win, filled = ref_pad.padded_window(img, y0, x0, size[0], size[1], ref_pad.NONE if mode is None else mode, fill3 if space == "pixel" else (0, 0, 0))
        val = rr.finish(win, mean, std, tname(torch, dtype))
        if space == "output":
            for ch in range(3):
                val[ch][filled] = rounded(torch, fill3[ch], dtype)
        out.append(val[:, :, ::-1] if flip is not None and flip[b] else val)
    return np.stack(out).astype(np.float32)


def nhwc_memory(torch, t):
    """the elements of a channels-last tensor in MEMORY order, as float32 on the host"""
    n, ch, h, w = t.shape
    assert ch == 3 and tuple(t.stride()) == (3 * h * w, 1, 3 * w, 3), (tuple(t.shape), tuple(t.stride()))
    return torch.as_strided(t, (n * h * w * 3,), (1,)).float().cpu().numpy()


def assert_tensor(torch, got, want, channels_last, what):
    """got (device tensor [B, 3, Ho, Wo] in either layout) holds `want`'s values bit for bit -- in the NHWC case read from memory, element
    (b, i, j, c) at ((b Ho + i) Wo + j) 3 + c, against the CPU tensor permuted"""
    assert tuple(got.shape) == want.shape, (what, tuple(got.shape), want.shape)
    if channels_last:
        mem = nhwc_memory(torch, got)
        ref = np.ascontiguousarray(want.transpose(0, 2, 3, 1)).reshape(-1)
    else:
        assert got.is_contiguous(), what
        mem, ref = got.float().cpu().numpy().reshape(-1), want.reshape(-1)
    same = mem.view(np.uint32) == ref.view(np.uint32)
    assert same.all(), (what, int((~same).sum()), "elements differ; first at", int(np.argmax(~same)), mem[~same][:4], ref[~same][:4])


def decode(c, bt, size, **kw):
    c.poison_workspace(POISON)
    out = c.decode_tensor(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size=size, **kw)
    c.check()
    assert (c.image_status(len(bt.sizes)) == 0).all()
    return out


def inside_origins(sizes, size, reduce=0):
    from llicti_amd.codec import reduced_dims
    rs = [reduce] * len(sizes) if isinstance(reduce, int) else reduce
    dims = [reduced_dims(h, w, r) for (h, w), r in zip(sizes, rs)]
    return ([min(h - size[0], 1 + 2 * b) for b, (h, _) in enumerate(dims)], [min(w - size[1], 3 + 2 * b) for b, (_, w) in enumerate(dims)])


# ------------------------------------------------------------------------------------------------ 1. NHWC, windows
@pytest.mark.parametrize("size", [(32, 32), (31, 29)])
@pytest.mark.parametrize("nlev,name,sizes", [(5, "auto", [(67, 93)] * 2), (5, "xrans3", [(64, 96)] * 2), (5, "auto", MIXED), (5, "xrans3", MIXED),
                                             (5, "ac", [(64, 96)] * 2), (2, "xrans2", MIXED)])
def test_nhwc_windows(torch_mod, codecs, nlev, name, sizes, size):
    """Windows inside their images in channels_last: the three dtypes, two mean / std pairs and none, flips, origins that differ per image --
    the CPU tensor permuted to NHWC, bit for bit; the returned strides; (identity) .contiguous() of it is the planar call's tensor."""
    torch = torch_mod
    c = codecs(nlev)
    bt = batch(torch, c, nlev, name, sizes)
    B = len(sizes)
    origin = inside_origins(sizes, size)
    flips = [None, [b % 2 for b in range(B)], [1] * B]
    k = 0
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        for mean, std in (IMAGENET, AWKWARD, (None, None)):
            flip = flips[k % 3]
            k += 1
            kw = dict(dtype=dt, origin=origin, flip=flip, mean=mean, std=std)
            got = decode(c, bt, size, channels_last=True, **kw)
            assert got.dtype == dt and tuple(got.shape) == (B, 3, *size) and tuple(got.stride()) == (3 * size[0] * size[1], 1, 3 * size[1], 3)
            assert got.is_contiguous(memory_format=torch.channels_last)
            assert_tensor(torch, got, expect(torch, bt, size, **kw), True, (dt, mean, flip))
            planar = decode(c, bt, size, **kw)                                   # (identity)
            assert torch.equal(got.contiguous().view(torch.uint8), planar.view(torch.uint8)), (dt, mean, flip)
    got = decode(c, bt, size, channels_last=True)                                # every default: the corner, float32
    assert_tensor(torch, got, expect(torch, bt, size), True, "defaults")


@pytest.mark.parametrize("size", [(16, 20), (15, 13)])
def test_nhwc_windows_of_a_reduced_decode(torch_mod, codecs, size):
    """reduce 2 on both batches (origins in the decimated grid), and the mixed batch with image 0 at reduce 0 and image 1 at reduce 1."""
    torch = torch_mod
    c = codecs(5)
    for sizes, reduce in (([(67, 93)] * 2, 2), (MIXED, 2), (MIXED, [0, 1])):
        bt = batch(torch, c, 5, "auto", sizes)
        origin = inside_origins(sizes, size, reduce)
        for dt, (mean, std), flip in ((torch.float16, IMAGENET, [1, 0]), (torch.float32, AWKWARD, None)):
            kw = dict(dtype=dt, origin=origin, flip=flip, mean=mean, std=std, reduce=reduce)
            got = decode(c, bt, size, channels_last=True, **kw)
            assert_tensor(torch, got, expect(torch, bt, size, **kw), True, (sizes, reduce, dt))


# ------------------------------------------------------------------------------------------------ 2. NHWC, resized and views
def _boxes():
    return [(3, 8, 140, 120), (10, 20, 70, 131)]


@pytest.mark.parametrize("antialias", [True, False])
def test_nhwc_resized(torch_mod, codecs, antialias):
    torch = torch_mod
    c = codecs(5)
    bt = batch(torch, c, 5, "auto", MIXED)
    size, boxes, flip = (40, 40), _boxes(), [0, 1]
    for dt in (torch.float16, torch.float32):
        c.poison_workspace(POISON)
        got = c.decode_tensor_resized(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size, boxes, dtype=dt, flip=flip, mean=IMAGENET[0], std=IMAGENET[1],
                                      antialias=antialias, channels_last=True)
        c.check()
        want = np.stack([rr.resized_crop(bt.rgbs[b], boxes[b], size, int(antialias), bool(flip[b]), *IMAGENET, tname(torch, dt)) for b in range(2)])
        assert_tensor(torch, got, want, True, (antialias, dt))
    # an odd width (element-wise stores), per-image reduce: box 1 on image 1's grid at reduce 1
    got = c.decode_tensor_resized(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, (17, 19), [(3, 8, 60, 70), (5, 10, 35, 65)], dtype=torch.bfloat16, antialias=antialias,
                                  reduce=[0, 1], channels_last=True)
    c.check()
    want = np.stack([rr.resized_crop(bt.rgbs[0], (3, 8, 60, 70), (17, 19), int(antialias), False, None, None, "bfloat16"),
                     rr.resized_crop(bt.rgbs[1][:, ::2, ::2], (5, 10, 35, 65), (17, 19), int(antialias), False, None, None, "bfloat16")])
    assert_tensor(torch, got, want, True, (antialias, "17x19 per-image reduce"))


def test_nhwc_views(torch_mod, codecs):
    """Two groups -- (32, 32) x 2 views per image and (17, 19) x 3 views per image -- with repeats, and an image no view names."""
    torch = torch_mod
    c = codecs(5)
    sizes = MIXED + [(64, 96)]
    bt = batch(torch, c, 5, "xrans3", sizes)
    g0 = dict(size=(32, 32), image=[0, 1, 0, 1], boxes=[(3, 8, 100, 120), (0, 20, 96, 128), (50, 3, 64, 64), (10, 0, 32, 32)], flip=[0, 1, 1, 0], dtype=torch.float16)
    g1 = dict(size=(17, 19), image=[1, 1, 0, 0, 1, 0], boxes=[(40, 50, 30, 30), (40, 50, 30, 30), (100, 90, 50, 41), (0, 0, 17, 19), (1, 2, 60, 70), (7, 7, 68, 76)],
              antialias=False)
    c.poison_workspace(POISON)
    outs = c.decode_tensor_views(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, [g0, g1], mean=IMAGENET[0], std=IMAGENET[1], channels_last=True)
    c.check()
    assert (c.image_status(3) == 0).all()
    for g, out in zip((g0, g1), outs):
        dt = g.get("dtype", torch.float32)
        want = np.stack([rr.resized_crop(bt.rgbs[b], box, g["size"], int(g.get("antialias", True)), bool(f), *IMAGENET, tname(torch, dt))
                         for b, box, f in zip(g["image"], g["boxes"], g.get("flip") or [0] * len(g["image"]))])
        assert_tensor(torch, out, want, True, g["size"])


# ------------------------------------------------------------------------------------------------ 3. padding
def _pad_windows(Hr, Wr, mode):
    """(name, size, (y0, x0)) on an Hr x Wr grid: each side alone, all four at once, exactly one pixel over an edge, at the mode's limit"""
    wins = [("top", (32, 32), (-5, 7)), ("left, 4-pixel pieces aligned", (32, 32), (4, -8)), ("bottom", (32, 32), (Hr - 20, 9)), ("left", (32, 32), (3, -9)), ("right", (32, 32), (5, Wr - 13)),
            ("all four", (Hr + 13, Wr + 19), (-6, -9)), ("one over, top left", (31, 29), (-1, -1)), ("one over, bottom right", (31, 29), (Hr - 30, Wr - 28))]
    if mode == "reflect":
        wins += [("limit, front", (Hr, Wr), (-(Hr - 1), -(Wr - 1))), ("limit, behind", (Hr, Wr), (Hr - 1, Wr - 1))]
    if mode == "symmetric":
        wins += [("limit, front", (Hr, Wr), (-Hr, -Wr)), ("limit, behind", (Hr, Wr), (Hr, Wr))]
    if mode in ("constant", "edge"):
        wins += [("wholly outside, above left", (31, 29), (-40, -50)), ("wholly outside, below", (32, 32), (Hr + 3, 4)), ("far outside", (8, 12), (8160, -8160))]
    return wins


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("mode", PAD_MODES)
@pytest.mark.parametrize("H,W", [(67, 93), (64, 96)])
def test_padded_windows(torch_mod, codecs, H, W, mode, channels_last):
    torch = torch_mod
    c = codecs(5)
    bt = batch(torch, c, 5, "auto", [(H, W)] * 2)
    fills = [dict(fill=(0, 0, 0), space="pixel"), dict(fill=(124, 116, 104), space="pixel"), dict(fill=0.0, space="output")]
    for k, (what, size, (y0, x0)) in enumerate(_pad_windows(H, W, mode)):
        origin = ([y0, y0], [x0, x0])
        for flip in (None, [1, 0]):
            f = fills[(k + (flip is not None)) % 3]
            dt = (torch.float32, torch.float16, torch.bfloat16)[k % 3]
            kw = dict(dtype=dt, origin=origin, flip=flip, mean=IMAGENET[0], std=IMAGENET[1])
            got = decode(c, bt, size, channels_last=channels_last, pad=dict(mode=mode, **f), **kw)
            assert_tensor(torch, got, expect(torch, bt, size, mode=mode, **f, **kw), channels_last, (what, flip, f, dt))
    # a fill in output space under normalisation is exactly 0 where the window leaves the image, in every dtype
    if mode == "constant":
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            got = decode(c, bt, (80, 112), channels_last=channels_last, dtype=dt, origin=([-6, -6], [-9, -9]), mean=AWKWARD[0], std=AWKWARD[1],
                         pad=dict(mode="constant", fill=0.0, space="output"))
            x = got.float().cpu().numpy()
            assert (x[:, :, :6, :] == 0).all() and (x[:, :, 6 + H:, :] == 0).all() and (x[:, :, :, :9] == 0).all() and (x[:, :, :, 9 + W:] == 0).all()
            assert not np.signbit(x[:, :, :6, :]).any()
            assert_tensor(torch, got, expect(torch, bt, (80, 112), origin=([-6, -6], [-9, -9]), mode="constant", fill=0.0, space="output", mean=AWKWARD[0],
                                             std=AWKWARD[1], dtype=dt), channels_last, ("output zero", dt))


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("mode", PAD_MODES)
def test_padded_windows_of_reduced_and_mixed_batches(torch_mod, codecs, mode, channels_last):
    """reduce = 2 (origins in the decimated grid: 17 x 24), and the mixed batch with each image at its own reduce -- one window overhangs its image
    on every side, the other lies across a corner; per-image fills of both spaces."""
    torch = torch_mod
    c = codecs(5)
    bt = batch(torch, c, 5, "auto", [(67, 93)] * 2)
    for size, origin in (((20, 28), ([-2, -1], [-3, 0])), ((9, 11), ([12, -4], [-5, 18]))):
        kw = dict(dtype=torch.float16, origin=origin, flip=[0, 1], mean=IMAGENET[0], std=IMAGENET[1], reduce=2)
        got = decode(c, bt, size, channels_last=channels_last, pad=dict(mode=mode, fill=(124, 116, 104)), **kw)
        assert_tensor(torch, got, expect(torch, bt, size, mode=mode, fill=(124, 116, 104), **kw), channels_last, ("reduce 2", size))
    bt = batch(torch, c, 5, "auto", MIXED)
    for reduce in ([0, 1], [2, 0]):
        for size, origin in (((64, 60), ([-7, -9], [100, -11])), ((33, 35), ([130, 40], [-20, 70]))):
            kw = dict(dtype=torch.float32, origin=origin, flip=[1, 0], mean=AWKWARD[0], std=AWKWARD[1], reduce=reduce)
            if not all(ref_pad.window_ok(*_grid(bt, b, reduce), origin[0][b], origin[1][b], *size, mode) for b in range(2)):
                assert mode in ("reflect", "symmetric")
                continue                      # (a window this mode does not mirror on this grid: the refusals are test_refusals')
            got = decode(c, bt, size, channels_last=channels_last, pad=dict(mode=mode, fill=0.25, space="output"), **kw)
            assert_tensor(torch, got, expect(torch, bt, size, mode=mode, fill=0.25, space="output", **kw), channels_last, ("mixed", reduce, size))


def _grid(bt, b, reduce):
    from llicti_amd.codec import reduced_dims
    return reduced_dims(bt.Hs[b], bt.Ws[b], reduce[b])


@pytest.mark.parametrize("nlev,name,sizes", [(5, "ac", [(64, 96)] * 2), (2, "xrans2", MIXED), (5, "xrans3", [(67, 93)] * 2)])
def test_padded_windows_other_models(torch_mod, codecs, nlev, name, sizes):
    """The reference format, config B and a fixed xwide count: one window over every side per mode, both layouts."""
    torch = torch_mod
    c = codecs(nlev)
    bt = batch(torch, c, nlev, name, sizes)
    size = (min(h for h, _ in sizes) + 10, min(w for _, w in sizes) + 12)
    origin = ([-5] * 2, [-6] * 2)
    for mode in PAD_MODES:
        for cl in (False, True):
            kw = dict(dtype=torch.bfloat16, origin=origin, flip=[0, 1], mean=IMAGENET[0], std=IMAGENET[1])
            if not all(ref_pad.window_ok(h, w, -5, -6, *size, mode) for h, w in sizes):
                continue
            got = decode(c, bt, size, channels_last=cl, pad=dict(mode=mode, fill=(124, 116, 104)), **kw)
            assert_tensor(torch, got, expect(torch, bt, size, mode=mode, fill=(124, 116, 104), **kw), cl, (name, mode, cl))


@pytest.mark.parametrize("size", [(32, 32), (31, 29)])
def test_a_window_inside_gives_the_unpadded_bytes(torch_mod, codecs, size):
    torch = torch_mod
    c = codecs(5)
    bt = batch(torch, c, 5, "auto", MIXED)
    origin = inside_origins(MIXED, size)
    for dt in (torch.float32, torch.float16):
        kw = dict(dtype=dt, origin=origin, flip=[0, 1], mean=IMAGENET[0], std=IMAGENET[1])
        plain = decode(c, bt, size, **kw)
        assert_tensor(torch, plain, expect(torch, bt, size, **kw), False, "unpadded")
        for mode in PAD_MODES:
            got = decode(c, bt, size, pad=dict(mode=mode, fill=(9, 8, 7)), **kw)
            assert torch.equal(got.view(torch.uint8), plain.view(torch.uint8)), (mode, dt)


# ------------------------------------------------------------------------------------------------ 4. nothing outside the tensor
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("size", [(32, 32), (31, 29)])
def test_nothing_outside_the_tensor(torch_mod, codecs, size, channels_last):
    """`out` is a view into a larger buffer of 0xA5, at an offset that keeps the wide stores (64 bytes) and at one that forbids them (one element):
    the bytes in front of and behind the tensor keep their value, and both offsets hold the same values -- padded windows and windows inside."""
    torch = torch_mod
    c = codecs(5)
    bt = batch(torch, c, 5, "auto", MIXED)
    Ho, Wo = size
    n = 2 * 3 * Ho * Wo
    strides = (3 * Ho * Wo, 1, 3 * Wo, 3) if channels_last else (3 * Ho * Wo, Ho * Wo, Wo, 1)
    for pad, origin in ((dict(mode="symmetric"), ([-3, 70], [110, -2])), (None, inside_origins(MIXED, size))):
        if pad is None and not channels_last:
            continue                          # (the sibling call: tests/test_hip_tensor.py)
        for dt in (torch.float32, torch.float16):
            es = torch.empty((), dtype=dt).element_size()
            kw = dict(dtype=dt, origin=origin, flip=[0, 1], mean=IMAGENET[0], std=IMAGENET[1])
            want = expect(torch, bt, size, mode=None if pad is None else pad["mode"], **kw)
            for front in (64, es):
                big = torch.full((256 + front + n * es + 64,), POISON, dtype=torch.uint8, device=DEV)
                base = (-big.data_ptr()) % 256 + front
                out = torch.as_strided(big[base:base + n * es].view(dt), (2, 3, Ho, Wo), strides)
                assert out.data_ptr() == big.data_ptr() + base and out.data_ptr() % 16 == front % 16
                got = decode(c, bt, size, channels_last=channels_last, pad=pad, out=out, **kw)
                assert got.data_ptr() == out.data_ptr()
                host = big.cpu()
                assert (host[:base] == POISON).all() and (host[base + n * es:] == POISON).all(), (dt, front, pad)
                assert_tensor(torch, got, want, channels_last, (dt, front, pad))


def test_out_must_have_the_layouts_strides(torch_mod, codecs):
    torch = torch_mod
    c = codecs(5)
    bt = batch(torch, c, 5, "auto", MIXED)
    planar = torch.empty((2, 3, 32, 32), device=DEV)
    with pytest.raises(AssertionError):
        c.decode_tensor(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size=(32, 32), out=planar, channels_last=True)
    with pytest.raises(AssertionError):
        c.decode_tensor(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size=(32, 32), out=planar.contiguous(memory_format=torch.channels_last))
    c.check()


# ------------------------------------------------------------------------------------------------ 5. per call, not per plan
def test_fresh_options_every_call_hit_one_plan(torch_mod, codecs):
    torch = torch_mod
    c = codecs(5)
    bt = batch(torch, c, 5, "auto", MIXED)
    size = (48, 52)
    decode(c, bt, size, channels_last=True, pad=dict(mode="edge"), origin=([-1, 0], [0, -1]))      # warm-up: the plan of (sizes, mode, reduce 0)
    names = ("plan_builds", "plan_hits", "device_syncs", "device_allocs")
    before = {k: c.counter(k) for k in names}
    rng = np.random.default_rng(5)
    calls = []
    for k in range(8):
        origin = ([int(rng.integers(-40, h - 8)) for h, _ in MIXED], [int(rng.integers(-40, w - 8)) for _, w in MIXED])
        kw = dict(origin=origin, flip=[int(v) for v in rng.integers(0, 2, 2)], mean=IMAGENET[0], std=IMAGENET[1], dtype=(torch.float16, torch.float32)[k % 2])
        mode = PAD_MODES[k % 4]
        f = dict(fill=tuple(float(v) for v in rng.integers(0, 256, 3)), space=("pixel", "output")[(k // 2) % 2])
        cl = bool(k % 3)
        calls.append((kw, mode, f, cl, c.decode_tensor(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size=size, channels_last=cl, pad=dict(mode=mode, **f), **kw)))
    after = {k: c.counter(k) for k in names}
    assert after["plan_builds"] == before["plan_builds"] and after["plan_hits"] == before["plan_hits"] + 8, (before, after)
    assert after["device_syncs"] == before["device_syncs"] and after["device_allocs"] == before["device_allocs"], (before, after)
    c.check()
    for kw, mode, f, cl, out in calls:
        assert_tensor(torch, out, expect(torch, bt, size, mode=mode, **f, **kw), cl, (kw["origin"], mode, f, cl))
    # ... and that plan is the reduced decode's: the planar call on the same batch finds it
    c.decode_reduced(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, 0)
    c.check()
    assert c.counter("plan_builds") == after["plan_builds"] and c.counter("plan_hits") == after["plan_hits"] + 1


# ------------------------------------------------------------------------------------------------ 6. status
def test_status_words_as_after_a_planar_decode(torch_mod, codecs):
    torch = torch_mod
    from llicti_amd._lib import EFORMAT, LlictiError
    c = codecs(5)
    sizes = MIXED + [(64, 96)]
    bt = batch(torch, c, 5, "xrans3", sizes)
    bad = bt.cont.clone()
    bad[1, 0] = 0x95                                   # the retired v2 tag: a deterministic rejection
    c.decode_v(bad, bt.seg, bt.Hs, bt.Ws, bt.mode)
    with pytest.raises(LlictiError) as e:
        c.check()
    assert e.value.code == EFORMAT
    want = c.image_status(3).copy()
    assert list(want) == [0, EFORMAT, 0]
    c.check()
    size, origin = (70, 100), ([-3, 30, -3], [40, -2, -2])
    kw = dict(origin=origin, flip=[1, 0, 1], mean=IMAGENET[0], std=IMAGENET[1], dtype=torch.float16)
    exact = expect(torch, bt, size, mode="edge", **kw)
    for cl in (True, False):
        c.poison_workspace(POISON)
        got = c.decode_tensor(bad, bt.seg, bt.Hs, bt.Ws, bt.mode, size=size, channels_last=cl, pad=dict(mode="edge"), **kw)
        with pytest.raises(LlictiError) as e:
            c.check()
        assert e.value.code == EFORMAT
        assert np.array_equal(c.image_status(3), want)
        x = got.float().cpu().numpy()
        for b in (0, 2):
            assert np.array_equal(x[b].view(np.uint32), exact[b].view(np.uint32)), (cl, b)
        c.check()


# ------------------------------------------------------------------------------------------------ 7. refusals
def _raises(c, bt, size, **kw):
    from llicti_amd._lib import LlictiError
    with pytest.raises(LlictiError) as e:
        c.decode_tensor(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size=size, **kw)
    return e.value


def test_refusals_are_einval_and_launch_nothing(torch_mod, codecs):
    torch = torch_mod
    from llicti_amd._lib import EINVAL
    c = codecs(5)
    bt = batch(torch, c, 5, "auto", MIXED)                 # 150 x 131, 96 x 160
    size = (32, 32)
    decode(c, bt, size, channels_last=True)
    c.check()
    inf, nan = float("inf"), float("nan")
    refused = [
        (dict(pad=dict(mode="constant"), origin=([0, -8161], [0, 0])), "image 1"), (dict(pad=dict(mode="edge"), origin=([0, 0], [8161, 0])), "image 0"),
        (dict(size=(8161, 4), pad=dict(mode="constant")), None), (dict(size=(4, 8161), pad=dict(mode="edge"), channels_last=True), None),
        (dict(size=(0, 4), pad=dict(mode="edge")), None), (dict(size=(4, -1), channels_last=True), None),
        (dict(pad=dict(mode="reflect"), origin=([-31, -31], [0, -32])), None),                        # fine: an overhang of 31 and 32 on axes of 96 .. 160
        (dict(pad=dict(mode="reflect"), size=(100, 32), origin=([0, -96], [0, 0])), "image 1"),       # 96 rows: reflect mirrors 95
        (dict(pad=dict(mode="reflect"), size=(100, 32), origin=([0, 92], [0, 0])), "image 1"),        # rows 92 .. 191: 96 past the bottom
        (dict(pad=dict(mode="symmetric"), size=(32, 140), origin=([0, 0], [-132, 0])), "image 0"),    # 131 columns: symmetric mirrors 131
        (dict(pad=dict(mode="symmetric"), size=(32, 140), origin=([0, 0], [123, 0])), "image 0"),     # columns 123 .. 262: 132 past the right
        (dict(pad=dict(mode="reflect"), reduce=[5, 0], origin=([0, 0], [-5, 0])), "image 0"),         # 5 x 5 at reduce 5: reflect mirrors 4
        (dict(pad=dict(mode="constant", fill=(0, inf, 0))), None), (dict(pad=dict(mode="constant", fill=nan, space="output")), None),
        (dict(pad=dict(mode="edge", fill=-inf)), None),
        (dict(pad=dict(mode=9)), None), (dict(pad=dict(mode=-1)), None), (dict(pad=dict(mode="constant", space=2)), None),
        (dict(pad=dict(mode="constant", space=-1), channels_last=True), None),
        (dict(origin=([0, 65], [0, 0]), channels_last=True), "image 1"),                              # no pad mode: the window leaves image 1, as ever
        (dict(origin=([-1, 0], [0, 0]), channels_last=True), "image 0"),
        (dict(pad=dict(mode="edge"), dtype=7), None), (dict(pad=dict(mode="edge"), mean=IMAGENET[0]), None),
        (dict(pad=dict(mode="edge"), mean=IMAGENET[0], std=(0.2, 0.0, 0.2), channels_last=True), None),
    ]
    ok = refused.pop(6)
    before = {k: c.counter(k) for k in ("plan_builds", "plan_hits")}
    for kw, names in refused:
        kw = dict(kw)
        sz = kw.pop("size", size)
        if min(sz) < 1 or max(sz) > 4096:       # (a size no tensor is made for: the library is asked directly, through the binding)
            err = _raises_raw(c, bt, sz, kw)
        else:
            err = _raises(c, bt, sz, **kw)
        assert err.code == EINVAL, kw
        assert names is None or names in str(err), (kw, str(err))
    # the layout, which the Python layer cannot misname: through the binding
    for layout in (2, -1):
        assert _raises_raw(c, bt, size, dict(), layout=layout).code == EINVAL
    # a pad mode on the resized and views calls
    for name in ("resized", "views"):
        assert _raises_raw(c, bt, size, dict(pad=dict(mode="edge")), call=name).code == EINVAL
    assert {k: c.counter(k) for k in before} == before                         # no plan was looked up, let alone built
    c.check()                                                                  # nothing was launched or latched ...
    kw = dict(ok[0])
    got = decode(c, bt, size, **kw)                                            # ... and a valid call is exact
    assert_tensor(torch, got, expect(torch, bt, size, origin=kw["origin"], mode="reflect"), False, "valid")


def _raises_raw(c, bt, size, kw, layout=None, call="tensor"):
    """one of the three _o calls through the ctypes binding, with options the Python layer would not build -> the LlictiError"""
    import ctypes as C
    import torch
    from llicti_amd import _lib
    from llicti_amd import codec as cd
    kw = dict(kw)
    opts = cd._tensor_opts(kw.pop("channels_last", False) or layout is not None, kw.pop("pad", None))
    if layout is not None:
        opts.layout = layout
    B = len(bt.sizes)
    Hs, Ws = np.ascontiguousarray(bt.Hs, dtype=np.int32), np.ascontiguousarray(bt.Ws, dtype=np.int32)
    ws = c.workspace_v(Hs, Ws, bt.mode)
    modes = np.ascontiguousarray([bt.mode] * B if isinstance(bt.mode, int) else bt.mode, dtype=np.int32)
    rv = np.zeros(B, dtype=np.int32)
    out = torch.empty((B * 3 * 64 * 64,), device=DEV)
    p = cd._ptr
    head = (c.ctx, p(bt.cont), bt.cont.shape[1], p(bt.seg), B, p(Hs), p(Ws), p(modes), B, p(rv), p(ws), ws.numel())
    stream = cd._stream_ptr(c.device)
    with pytest.raises(_lib.LlictiError) as e:
        if call == "tensor":
            _lib.check(c.L.llicti_decode_images_tensor_o(*head, p(out), 0, int(size[0]), int(size[1]), None, None, None, None, None, stream, C.byref(opts)))
        elif call == "resized":
            _lib.check(c.L.llicti_decode_images_tensor_resized_o(*head, p(out), 0, 32, 32, None, None, None, None, None, None, None, 1, stream, C.byref(opts)))
        else:
            g = (_lib.ViewGroup * 1)()
            g[0].d_out, g[0].dtype, g[0].Ho, g[0].Wo, g[0].antialias, g[0].n = out.data_ptr(), 0, 32, 32, 1, B
            _lib.check(c.L.llicti_decode_images_tensor_views_o(*head, g, 1, None, None, stream, C.byref(opts)))
    return e.value


def test_null_options_are_the_sibling_call(torch_mod, codecs):
    """opts = NULL, and { NCHW, PAD_NONE } with garbage in the unread fields: the _rv sibling's bytes and counters."""
    import ctypes as C
    torch = torch_mod
    from llicti_amd import _lib
    from llicti_amd import codec as cd
    c = codecs(5)
    bt = batch(torch, c, 5, "auto", MIXED)
    size, origin, flip = (31, 29), inside_origins(MIXED, (31, 29)), [1, 0]
    want = decode(c, bt, size, origin=origin, flip=flip, mean=IMAGENET[0], std=IMAGENET[1], dtype=torch.float16)
    assert_tensor(torch, want, expect(torch, bt, size, origin=origin, flip=flip, mean=IMAGENET[0], std=IMAGENET[1], dtype=torch.float16), False, "sibling")
    B = 2
    Hs, Ws = np.ascontiguousarray(bt.Hs, dtype=np.int32), np.ascontiguousarray(bt.Ws, dtype=np.int32)
    ws = c.workspace_v(Hs, Ws, bt.mode)
    modes = np.ascontiguousarray([bt.mode] * B if isinstance(bt.mode, int) else bt.mode, dtype=np.int32)
    rv = np.zeros(B, dtype=np.int32)
    y0, x0 = (np.ascontiguousarray(v, dtype=np.int32) for v in origin)
    fl, mn, sd = np.ascontiguousarray(flip, dtype=np.uint8), np.ascontiguousarray(IMAGENET[0], dtype=np.float32), np.ascontiguousarray(IMAGENET[1], dtype=np.float32)
    p = cd._ptr
    names = ("plan_builds", "plan_hits", "device_syncs", "device_allocs", "block_waits")

    def run(fn, *tail):
        out = torch.full((B, 3, *size), float("nan"), dtype=torch.float16, device=DEV)
        c.poison_workspace(POISON)
        before = {k: c.counter(k) for k in names}
        _lib.check(fn(c.ctx, p(bt.cont), bt.cont.shape[1], p(bt.seg), B, p(Hs), p(Ws), p(modes), B, p(rv), p(ws), ws.numel(), p(out), cd.T_F16, size[0], size[1],
                      p(y0), p(x0), p(fl), p(mn), p(sd), cd._stream_ptr(c.device), *tail))
        c.check()
        return out, {k: c.counter(k) - before[k] for k in names}
    sib, d_sib = run(c.L.llicti_decode_images_tensor_rv)
    assert torch.equal(sib.view(torch.uint8), want.view(torch.uint8))
    plain = _lib.TensorOpts(cd.LAYOUT_NCHW, cd.PAD_NONE, 77, (float("nan"), 1e30, -1.0))
    for tail in ((None,), (C.byref(plain),)):
        got, d = run(c.L.llicti_decode_images_tensor_o, *tail)
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)) and d == d_sib, (tail, d, d_sib)


# ------------------------------------------------------------------------------------------------ 8. a caller's stream
def test_on_a_callers_stream_behind_a_gate(torch_mod, codecs):
    """One padded NHWC call on a caller's non-blocking stream that a gate (helpers.StreamGate) holds busy: the containers it reads are DECOYS until
    a copy, enqueued on that stream behind the gate, overwrites them; the output is poison until the call writes it and is copied out on the
    stream.  Everything is enqueued before the gate ends (asserted), so a launch not ordered on the stream would have decoded the decoys."""
    torch = torch_mod
    c = codecs(5)
    bt = batch(torch, c, 5, "auto", MIXED)
    decoy = batch(torch, c, 5, "auto", MIXED, seed=900)
    assert bt.cont.shape == decoy.cont.shape and not torch.equal(bt.cont, decoy.cont) and bt.mode == decoy.mode
    size, origin = (64, 60), ([-7, 50], [90, -11])
    kw = dict(dtype=torch.float16, origin=origin, flip=[1, 0], mean=IMAGENET[0], std=IMAGENET[1])
    pad = dict(mode="symmetric")
    want = expect(torch, bt, size, mode="symmetric", **kw)
    s = torch.cuda.Stream(device=DEV)
    gate = StreamGate(torch, DEV)
    with torch.cuda.stream(s):                          # warm on this stream: kernels loaded, plan cached, workspace there
        decode(c, bt, size, channels_last=True, pad=pad, **kw)
    torch.cuda.synchronize()
    cont, seg = decoy.cont.clone(), decoy.seg.clone()
    out = torch.full((2, 3, *size), float("nan"), dtype=torch.float16, device=DEV).contiguous(memory_format=torch.channels_last)
    c.poison_workspace(POISON)
    torch.cuda.synchronize()
    begin, end = gate.hold(s, 100.0)
    with torch.cuda.stream(s):
        cont.copy_(bt.cont, non_blocking=True)
        seg.copy_(bt.seg, non_blocking=True)
        c.decode_tensor(cont, seg, bt.Hs, bt.Ws, bt.mode, size=size, channels_last=True, pad=pad, out=out, **kw)
        got = torch.empty_like(out)
        got.copy_(out, non_blocking=True)
    assert not end.query(), "the gate ended before the last enqueue: the run proves nothing"
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c.check()
    assert_tensor(torch, got, want, True, "gated")


# ------------------------------------------------------------------------------------------------ 9. the model layer
def test_model_layer_center_crop(torch_mod):
    """LLICTI.decode_batch_async(tensor=dict(size=(48, 48), origin=center_crop_origins(...), pad=dict(mode="constant"), channels_last=True, ...)) on
    the mixed batch plus a 40 x 60 image, against CenterCrop(48) + ToTensor + Normalize restated on the CPU: pad where the image is smaller, cut
    from the middle, / 255, normalise."""
    torch = torch_mod
    from llicti_amd.codec import center_crop_origins
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    torch.manual_seed(1337)
    m = LLICTI(default_config(container="auto")).to(DEV).eval()
    dev = torch.device(DEV)
    sizes = MIXED + [(40, 60)]
    rgbs = [make_image("smooth", h, w, 40 + i) for i, (h, w) in enumerate(sizes)]
    lists = m.encode_batch_async(rgbs).lists()
    origin = center_crop_origins(sizes, (48, 48))
    assert origin == ([51, 24, -4], [42, 56, 6])
    m.codec().poison_workspace()
    got = m.decode_batch_async(lists, dev, tensor=dict(size=(48, 48), origin=origin, pad=dict(mode="constant"), channels_last=True, mean=IMAGENET[0], std=IMAGENET[1]))
    m.codec().check()
    want = []
    for img in rgbs:                                      # torchvision's CenterCrop.forward, on the uint8 image
        _, h, w = img.shape
        if h < 48 or w < 48:
            top, left = ((48 - h) // 2 if h < 48 else 0), ((48 - w) // 2 if w < 48 else 0)
            bottom, right = ((48 - h + 1) // 2 if h < 48 else 0), ((48 - w + 1) // 2 if w < 48 else 0)
            img = np.pad(img, ((0, 0), (top, bottom), (left, right)), mode="constant", constant_values=0)
            _, h, w = img.shape
        top, left = int(round((h - 48) / 2.0)), int(round((w - 48) / 2.0))
        x = torch.from_numpy(img[:, top:top + 48, left:left + 48].copy()).float() / 255
        mean, std = torch.tensor(IMAGENET[0]), torch.tensor(IMAGENET[1])
        want.append(((x - mean[:, None, None]) / std[:, None, None]).numpy())
    assert_tensor(torch, got, np.stack(want), True, "CenterCrop(48)")
