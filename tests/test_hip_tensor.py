"""Float tensors on the GPU (run with -m gpu on an MI355X): llicti_decode_images_tensor writes the dense [B, 3, Ho, Wo] float32 / float16 /
bfloat16 tensor a network is fed with -- crop, horizontal flip, mean / std -- from the decode's last kernel, llicti_encode_images_f32 reads planar
float32 in {k/255}.  Every check is EXACT (torch.equal / np.array_equal, no tolerance).  The yardsticks are the planar uint8 calls (decode /
decode_v / decode_reduced / encode / encode_v, themselves pinned to the oracle) and the arithmetic spec of include/llicti_hip.h evaluated by
PyTorch ON THE CPU on the uint8 pixels: v / 255, (x - mean) / std, .to(dtype).  The shapes are those of test_hip_pixel_formats.py, the smallest
that reach every form of the row walk: 32x32, 33x35 and 67x93 (W % 4 != 0), 64x96 (4-element stores and loads), and a mixed batch."""
import numpy as np
import pytest

from conftest import load_state_dict
from helpers import make_image

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32), (33, 35), (67, 93), (64, 96)]
MIXED = [(67, 93), (64, 96), (33, 35)]
MODELS = [(5, "xrans2"), (5, "ac"), (5, "auto"), (2, "xrans2")]      # (levels, container); "ac" codes equal sizes only
MODELS_MIXED = [m for m in MODELS if m[1] != "ac"]
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
AWKWARD = ((0.1, 0.3337, 0.9), (0.007, 1.0, 3.3))
POISON = 0xA5


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _new_codec(nlev):
    from llicti_amd.codec import HipCodec
    c = HipCodec("cuda:0")
    if nlev == 2:
        c.set_model(60, 2)
        c.load_state_dict(load_state_dict("b_trainedlike"))
    else:
        c.load_state_dict(load_state_dict("trainedlike"))
    return c


@pytest.fixture(scope="module")
def codecs(torch_mod):
    cache = {}

    def get(nlev=5):
        if nlev not in cache:
            cache[nlev] = _new_codec(nlev)
        return cache[nlev]
    yield get
    for c in cache.values():
        c.close()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _enc_mode(name, sizes, nlev):
    from llicti_amd.codec import auto_modes, mode_of_name
    if name != "auto":
        return mode_of_name(name)
    modes = auto_modes(sizes, nlev)
    return modes[0] if all(m == modes[0] for m in modes) else modes


class Batch:
    """One encoded batch and its yardstick, made once per (model, container, sizes): the containers on the device, the mode a decoder takes for
    them, and the FULL planar uint8 decode of every image on the host (decode for equal sizes, decode_v for mixed ones)."""

    def __init__(self, torch, c, nlev, name, sizes, seed):
        self.sizes = list(sizes)
        self.Hs, self.Ws = [h for h, _ in sizes], [w for _, w in sizes]
        rgbs = [make_image(("smooth", "noise")[i % 2], h, w, seed + i) for i, (h, w) in enumerate(sizes)]
        enc = _enc_mode(name, self.sizes, nlev)
        self.uniform = len(set(self.sizes)) == 1
        if self.uniform:
            self.cont, self.seg = c.encode(_dev(torch, np.stack(rgbs)), mode=enc if isinstance(enc, int) else enc[0])
        else:
            self.cont, self.seg = c.encode_v(_dev(torch, np.concatenate([r.reshape(-1) for r in rgbs])), self.Hs, self.Ws, enc)
        c.check()
        modes = c.container_modes(self.cont)          # (what the headers say: an "auto" encoder mode is no decoder's mode)
        self.mode = modes[0] if all(m == modes[0] for m in modes) else modes
        c.poison_workspace(POISON)
        if self.uniform:
            full = c.decode(self.cont, self.seg, self.Hs[0], self.Ws[0], mode=self.mode).cpu()
            self.u8 = [full[b] for b in range(len(sizes))]
        else:
            flat = c.decode_v(self.cont, self.seg, self.Hs, self.Ws, self.mode).cpu()
            offs, _ = c.flat_offsets(self.Hs, self.Ws)
            self.u8 = [flat[int(o):int(o) + 3 * h * w].view(3, h, w) for o, (h, w) in zip(offs, sizes)]
        c.check()
        for got, want in zip(self.u8, rgbs):
            assert np.array_equal(got.numpy(), want)      # (the yardstick is what it should be)
        self._reduced = {}

    def reduced(self, c, r):
        """the planar uint8 images at reduce r (decode_reduced), on the host"""
        from llicti_amd.codec import reduced_dims
        if r not in self._reduced:
            flat = c.decode_reduced(self.cont, self.seg, self.Hs, self.Ws, self.mode, r).cpu()
            c.check()
            out, pos = [], 0
            for h, w in self.sizes:
                hr, wr = reduced_dims(h, w, r)
                out.append(flat[pos:pos + 3 * hr * wr].view(3, hr, wr))
                pos += 3 * hr * wr
            self._reduced[r] = out
        return self._reduced[r]


_BATCHES = {}


def batch(torch, c, nlev, name, sizes, seed=700):
    key = (nlev, name, tuple(sizes), seed)
    if key not in _BATCHES:
        _BATCHES[key] = Batch(torch, c, nlev, name, sizes, seed)
    return _BATCHES[key]


def spec(torch, u8, mean=None, std=None, dtype=None):
    """The arithmetic spec on the CPU: uint8 [.., 3, h, w] -> v / 255, then (x - mean[c]) / std[c], then .to(dtype)."""
    assert u8.dtype == torch.uint8 and not u8.is_cuda
    x = u8.float() / 255
    if mean is not None:
        m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
        x = (x - m[:, None, None]) / s[:, None, None]
    return x if dtype is None else x.to(dtype)


def crops(torch, imgs, size, origin=None, flip=None):
    """uint8 images [3, h_b, w_b] -> uint8 [B, 3, Ho, Wo]: every image's window, mirrored where flagged"""
    Ho, Wo = size
    out = []
    for b, im in enumerate(imgs):
        y0, x0 = (0, 0) if origin is None else (int(origin[0][b]), int(origin[1][b]))
        win = im[:, y0:y0 + Ho, x0:x0 + Wo]
        assert win.shape == (3, Ho, Wo)
        out.append(torch.flip(win, dims=[-1]) if flip is not None and flip[b] else win)
    return torch.stack(out)


def decode_tensor(c, bt, size, **kw):
    c.poison_workspace(POISON)
    out = c.decode_tensor(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size=size, **kw)
    c.check()
    assert (c.image_status(len(bt.sizes)) == 0).all()
    return out


def origin_sets(sizes, size):
    """(every window at the corner, every window at its largest legal origin, odd origins in between that differ per image)"""
    Ho, Wo = size
    last = ([h - Ho for h, _ in sizes], [w - Wo for _, w in sizes])
    odd = ([min(h - Ho, 1 + 2 * b) for b, (h, _) in enumerate(sizes)], [min(w - Wo, 1 + 2 * ((b + 1) % 3)) for b, (_, w) in enumerate(sizes)])
    return [([0] * len(sizes), [0] * len(sizes)), last, odd]


# ------------------------------------------------------------------------------------------------ 1. full window, float32
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("nlev,name", MODELS)
def test_full_window_f32(torch_mod, codecs, nlev, name, H, W):
    torch = torch_mod
    c = codecs(nlev)
    bt = batch(torch, c, nlev, name, [(H, W)] * 2)
    got = decode_tensor(c, bt, (H, W))
    assert got.dtype == torch.float32 and got.shape == (2, 3, H, W)
    assert torch.equal(got.cpu(), torch.stack(bt.u8).float() / 255)


# ------------------------------------------------------------------------------------------------ 2. normalisation, the three dtypes
@pytest.mark.parametrize("H,W", [(67, 93), (64, 96)])
@pytest.mark.parametrize("mean,std", [IMAGENET, AWKWARD])
def test_normalised_f32_f16_bf16(torch_mod, codecs, mean, std, H, W):
    torch = torch_mod
    c = codecs(5)
    bt = batch(torch, c, 5, "xrans2", [(H, W)] * 2)
    u8 = torch.stack(bt.u8)
    want = spec(torch, u8, mean, std)
    assert want.dtype == torch.float32
    got = decode_tensor(c, bt, (H, W), mean=mean, std=std)
    assert torch.equal(got.cpu(), want)
    for dt in (torch.float16, torch.bfloat16):
        got = decode_tensor(c, bt, (H, W), dtype=dt, mean=mean, std=std)
        assert got.dtype == dt and torch.equal(got.cpu(), want.to(dt)), dt
        got = decode_tensor(c, bt, (H, W), dtype=dt)                          # (and without normalisation)
        assert torch.equal(got.cpu(), spec(torch, u8, dtype=dt)), dt


# ------------------------------------------------------------------------------------------------ 3. + 4. crops of a mixed batch, flips
@pytest.mark.parametrize("size", [(32, 32), (31, 29)])
@pytest.mark.parametrize("nlev,name", MODELS_MIXED)
def test_crops_and_flips_of_a_mixed_batch(torch_mod, codecs, nlev, name, size):
    """Three images of three sizes into ONE [3, 3, Ho, Wo] tensor: 32x32 (4-element stores) and 31x29 (element by element), the windows at the
    corner, at the largest legal origin and at odd origins that differ per image; then the same with images 0 and 2 mirrored."""
    torch = torch_mod
    c = codecs(nlev)
    bt = batch(torch, c, nlev, name, MIXED)
    for origin in origin_sets(MIXED, size):
        for flip in (None, [1, 0, 1]):
            got = decode_tensor(c, bt, size, origin=origin, flip=flip, mean=IMAGENET[0], std=IMAGENET[1])
            assert got.shape == (3, 3, *size)
            assert torch.equal(got.cpu(), spec(torch, crops(torch, bt.u8, size, origin, flip), *IMAGENET)), (origin, flip)
    got = decode_tensor(c, bt, size, origin=origin_sets(MIXED, size)[2], flip=[1, 0, 1])
    assert torch.equal(got.cpu(), spec(torch, crops(torch, bt.u8, size, origin_sets(MIXED, size)[2], [1, 0, 1])))
    plain = crops(torch, bt.u8, size, origin_sets(MIXED, size)[2])
    assert torch.equal(got.cpu()[1], spec(torch, plain)[1]) and torch.equal(got.cpu()[0], torch.flip(spec(torch, plain)[0], dims=[-1]))


# ------------------------------------------------------------------------------------------------ 5. reduced
@pytest.mark.parametrize("nlev", [5, 2])
def test_windows_of_a_reduced_decode(torch_mod, codecs, nlev):
    """reduce = 1: 32x32 windows at the largest legal origins of 34x47 and 32x48; reduce = 2: 16x23 windows (odd width) of 17x24 and 16x24 at the
    corner and at odd origins, plain and mirrored -- slices of decode_reduced."""
    torch = torch_mod
    c = codecs(nlev)
    sizes = [(67, 93), (64, 96)]
    bt = batch(torch, c, nlev, "xrans2", sizes)
    red = bt.reduced(c, 1)
    assert [tuple(r.shape[1:]) for r in red] == [(34, 47), (32, 48)]
    origin = ([2, 0], [15, 16])
    for flip in (None, [0, 1]):
        got = decode_tensor(c, bt, (32, 32), origin=origin, flip=flip, reduce=1)
        assert torch.equal(got.cpu(), spec(torch, crops(torch, red, (32, 32), origin, flip))), flip
    red = bt.reduced(c, 2)
    assert [tuple(r.shape[1:]) for r in red] == [(17, 24), (16, 24)]
    for origin in (([0, 0], [0, 0]), ([1, 0], [1, 1])):
        for flip in (None, [1, 1]):
            got = decode_tensor(c, bt, (16, 23), origin=origin, flip=flip, reduce=2, dtype=torch.bfloat16, mean=AWKWARD[0], std=AWKWARD[1])
            assert torch.equal(got.cpu(), spec(torch, crops(torch, red, (16, 23), origin, flip), *AWKWARD, dtype=torch.bfloat16)), (origin, flip)


# ------------------------------------------------------------------------------------------------ 6. nothing outside the tensor
@pytest.mark.parametrize("size", [(32, 32), (31, 29)])
def test_nothing_outside_the_tensor(torch_mod, codecs, size):
    """`out` is a view into a larger buffer of 0xA5, at an offset that keeps 4-element stores (64 bytes) and at one that forbids them (one
    element): the bytes in front of and behind the tensor keep their value; the workspace is poisoned before every call."""
    torch = torch_mod
    c = codecs(5)
    bt = batch(torch, c, 5, "xrans2", MIXED)
    origin = origin_sets(MIXED, size)[2]
    n = 3 * 3 * size[0] * size[1]
    for dt in (torch.float32, torch.float16):
        es = torch.empty((), dtype=dt).element_size()
        for pad in (64, es):
            big = torch.full((pad + n * es + 64,), POISON, dtype=torch.uint8, device="cuda:0")
            out = big[pad:pad + n * es].view(dt).view(3, 3, *size)
            got = decode_tensor(c, bt, size, dtype=dt, origin=origin, flip=[0, 1, 1], out=out)
            assert got.data_ptr() == out.data_ptr() == big.data_ptr() + pad
            host = big.cpu()
            assert (host[:pad] == POISON).all() and (host[pad + n * es:] == POISON).all(), (dt, pad)
            assert torch.equal(host[pad:pad + n * es].view(dt).view(3, 3, *size), spec(torch, crops(torch, bt.u8, size, origin, [0, 1, 1]), dtype=dt)), (dt, pad)


# ------------------------------------------------------------------------------------------------ 7. the windows are per call
def test_new_windows_every_call_hit_one_plan(torch_mod, codecs):
    torch = torch_mod
    c = codecs(5)
    bt = batch(torch, c, 5, "xrans2", MIXED)
    size = (32, 32)
    decode_tensor(c, bt, size)                                                 # warm-up: the plan of (sizes, mode, reduce 0)
    before = {k: c.counter(k) for k in ("plan_builds", "plan_hits", "device_syncs", "device_allocs")}
    rng = np.random.default_rng(5)
    results = []
    for _ in range(8):
        origin = ([int(rng.integers(0, h - size[0] + 1)) for h, _ in MIXED], [int(rng.integers(0, w - size[1] + 1)) for _, w in MIXED])
        flip = [int(v) for v in rng.integers(0, 2, 3)]
        out = c.decode_tensor(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size=size, origin=origin, flip=flip, mean=IMAGENET[0], std=IMAGENET[1])
        results.append((origin, flip, out))
    after = {k: c.counter(k) for k in before}
    assert after["plan_builds"] == before["plan_builds"] and after["plan_hits"] == before["plan_hits"] + 8, (before, after)
    assert after["device_syncs"] == before["device_syncs"] and after["device_allocs"] == before["device_allocs"], (before, after)
    c.check()
    assert len({(tuple(o[0]), tuple(o[1]), tuple(f)) for o, f, _ in results}) > 1
    for origin, flip, out in results:
        assert torch.equal(out.cpu(), spec(torch, crops(torch, bt.u8, size, origin, flip), *IMAGENET)), (origin, flip)
    # ... and that plan is llicti_decode_images_reduced's: the planar call on the same batch finds it
    c.decode_reduced(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, 0)
    c.check()
    assert c.counter("plan_builds") == after["plan_builds"] and c.counter("plan_hits") == after["plan_hits"] + 1


# ------------------------------------------------------------------------------------------------ 8. status
def test_status_words_as_after_a_planar_decode(torch_mod, codecs):
    """Image 1's container gets an unknown tag in header byte 0 (a reported error, never a fault): decode_tensor latches the same per-image
    words as decode_v and reports LLICTI_EFORMAT; the other images are exact."""
    torch = torch_mod
    from llicti_amd._lib import EFORMAT, LlictiError
    c = codecs(5)
    bt = batch(torch, c, 5, "xrans2", MIXED)
    size = (32, 32)
    bad = bt.cont.clone()
    bad[1, 0] = 0x95                                   # the retired v2 tag: a deterministic rejection
    c.decode_v(bad, bt.seg, bt.Hs, bt.Ws, bt.mode)
    with pytest.raises(LlictiError) as e:
        c.check()
    assert e.value.code == EFORMAT
    want = c.image_status(3).copy()
    assert list(want) == [0, EFORMAT, 0]
    c.check()                                          # (read and cleared)
    c.poison_workspace(POISON)
    got = c.decode_tensor(bad, bt.seg, bt.Hs, bt.Ws, bt.mode, size=size, mean=IMAGENET[0], std=IMAGENET[1])
    with pytest.raises(LlictiError) as e:
        c.check()
    assert e.value.code == EFORMAT
    assert np.array_equal(c.image_status(3), want)
    exact = spec(torch, crops(torch, bt.u8, size), *IMAGENET)
    for b in (0, 2):
        assert torch.equal(got.cpu()[b], exact[b]), b
    c.check()
    assert torch.equal(decode_tensor(c, bt, size).cpu(), spec(torch, crops(torch, bt.u8, size)))      # a valid batch: clean status (decode_tensor checks it)


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_are_einval_and_launch_nothing(torch_mod, codecs):
    torch = torch_mod
    from llicti_amd._lib import EINVAL, LlictiError
    c = codecs(5)
    bt = batch(torch, c, 5, "xrans2", MIXED)
    size = (32, 32)
    last = origin_sets(MIXED, size)[1]
    decode_tensor(c, bt, size)
    c.check()
    row = ([last[0][0], last[0][1] + 1, last[0][2]], last[1])                  # image 1: one row too far
    col = (last[0], [last[1][0], last[1][1], last[1][2] + 1])                  # image 2: one column too far
    refused = [dict(origin=row), dict(origin=col), dict(origin=([-1, 0, 0], [0, 0, 0])),
               dict(reduce=1),                                                 # (33, 35) at reduce 1 is 17 x 18: no 32 x 32 window
               dict(mean=IMAGENET[0], std=(0.229, 0.0, 0.225)), dict(mean=IMAGENET[0], std=(0.229, -1.0, 0.225)),
               dict(mean=IMAGENET[0], std=(0.229, float("inf"), 0.225)), dict(mean=IMAGENET[0], std=(float("nan"), 1.0, 1.0)),
               dict(mean=IMAGENET[0]), dict(std=IMAGENET[1]),                  # one without the other
               dict(dtype=7), dict(dtype=-1)]
    before = {k: c.counter(k) for k in ("plan_builds", "plan_hits")}
    for kw in refused:
        with pytest.raises(LlictiError) as e:
            c.decode_tensor(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size=kw.pop("size", size), **kw)
        assert e.value.code == EINVAL, kw
    for bad_size in ((0, 32), (32, 0), (-3, 32)):
        with pytest.raises(LlictiError) as e:
            c.decode_tensor(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size=bad_size, out=torch.empty((3, 3, 32, 32), device="cuda:0"))
        assert e.value.code == EINVAL, bad_size
    assert "image 1" in str(_raises(c, bt, size, origin=row)) and "image 2" in str(_raises(c, bt, size, origin=col))
    assert {k: c.counter(k) for k in before} == before                         # no plan was looked up, let alone built
    c.check()                                                                  # nothing was launched or latched ...
    got = decode_tensor(c, bt, size, origin=last, mean=IMAGENET[0], std=IMAGENET[1])
    assert torch.equal(got.cpu(), spec(torch, crops(torch, bt.u8, size, last), *IMAGENET))      # ... and a valid call is exact


def _raises(c, bt, size, **kw):
    from llicti_amd._lib import LlictiError
    with pytest.raises(LlictiError) as e:
        c.decode_tensor(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size=size, **kw)
    return e.value


# ------------------------------------------------------------------------------------------------ 10. encode from float32
def _containers(c, cont, seg):
    c.check()
    seg = seg.cpu().numpy()
    return [cont[b, :int(seg[b].sum())].cpu().numpy() for b in range(seg.shape[0])], seg


def _assert_same(got, want, what):
    assert np.array_equal(got[1], want[1]), (what, "seg_len differs")
    for b, (g, w) in enumerate(zip(got[0], want[0])):
        assert np.array_equal(g, w), (what, b, "container bytes differ")


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("nlev,name", MODELS)
def test_encode_f32_gives_the_uint8_containers(torch_mod, codecs, nlev, name, H, W):
    """x = u8 / 255 built on the CPU: the containers and seg_len of encode_v on u8, byte for byte; the same for x + 0.3 / 255, which rounds back;
    and 1.5, -0.2 and a NaN code as 255, 0 and 0."""
    torch = torch_mod
    c = codecs(nlev)
    u8 = torch.from_numpy(make_image("smooth" if (H + W) % 2 else "noise", H, W, 900 + H + W))
    mode = _enc_mode(name, [(H, W)], nlev)
    want = _containers(c, *c.encode_v(u8.reshape(-1).to("cuda:0"), [H], [W], mode))
    x = u8.float() / 255
    _assert_same(_containers(c, *c.encode_f32(x.reshape(-1).to("cuda:0"), [H], [W], mode)), want, "k / 255")
    _assert_same(_containers(c, *c.encode_f32((x + 0.3 / 255).reshape(-1).to("cuda:0"), [H], [W], mode)), want, "k / 255 + 0.3 / 255")
    odd, v = x.clone(), u8.clone()
    for (ch, i, j), (f, k) in zip(((0, 0, 0), (1, H // 2, W - 1), (2, H - 1, 3), (0, 5, 6), (1, 31, 31)),
                                  ((1.5, 255), (-0.2, 0), (float("nan"), 0), (float("inf"), 255), (-float("inf"), 0))):
        odd[ch, i, j] = f
        v[ch, i, j] = k
    want = _containers(c, *c.encode_v(v.reshape(-1).to("cuda:0"), [H], [W], mode))
    _assert_same(_containers(c, *c.encode_f32(odd.reshape(-1).to("cuda:0"), [H], [W], mode)), want, "out of range, NaN")


@pytest.mark.parametrize("nlev,name", MODELS_MIXED)
def test_encode_f32_mixed_batch_with_gaps(torch_mod, codecs, nlev, name):
    """Three sizes in one call, back to back (x_off None) and at explicit element offsets with gaps of noise between the images -- one set of
    offsets that keeps 4-float loads possible where the plane size allows, one that is odd."""
    torch = torch_mod
    c = codecs(nlev)
    u8s = [torch.from_numpy(make_image(("smooth", "noise")[i % 2], h, w, 950 + i)) for i, (h, w) in enumerate(MIXED)]
    Hs, Ws = [h for h, _ in MIXED], [w for _, w in MIXED]
    mode = _enc_mode(name, MIXED, nlev)
    want = _containers(c, *c.encode_v(torch.cat([u.reshape(-1) for u in u8s]).to("cuda:0"), Hs, Ws, mode))
    xs = [u.float() / 255 for u in u8s]
    _assert_same(_containers(c, *c.encode_f32(torch.cat([x.reshape(-1) for x in xs]).to("cuda:0"), Hs, Ws, mode)), want, "back to back")
    for gap in (64, 37):
        offs, pos = [], gap
        for x in xs:
            offs.append(pos)
            pos += x.numel() + gap
        flat = torch.from_numpy(np.random.default_rng(gap).standard_normal(pos).astype(np.float32))
        for o, x in zip(offs, xs):
            flat[o:o + x.numel()] = x.reshape(-1)
        _assert_same(_containers(c, *c.encode_f32(flat.to("cuda:0"), Hs, Ws, mode, x_off=offs)), want, ("gaps", gap))


# ------------------------------------------------------------------------------------------------ 11. the model API
def _model(torch, container):
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    torch.manual_seed(1337)
    return LLICTI(default_config(container=container)).to("cuda:0").eval()


@pytest.mark.parametrize("container", ["ac", "auto"])
def test_model_round_trip_in_float(torch_mod, container):
    """encode_batch_async(x, pixels="f32") then decode_batch_async(..., tensor=dict(size=(H, W))) returns x exactly for x in {k/255}; the
    bytestream_lists are those of the uint8 call; a list of two sizes comes back as one cropped tensor."""
    torch = torch_mod
    m = _model(torch, container)
    dev = torch.device("cuda:0")
    H, W = 67, 93
    u8 = torch.from_numpy(np.stack([make_image("smooth", H, W, 30), make_image("noise", H, W, 31)]))
    x = (u8.float() / 255).to(dev)
    enc = m.encode_batch_async(x, pixels="f32")
    lists = enc.lists()
    assert lists == m.encode_batch_async(u8).lists() and (enc.Hs, enc.Ws) == ([H, H], [W, W])
    m.codec().poison_workspace()
    back = m.decode_batch_async(lists, dev, tensor=dict(size=(H, W)))
    m.codec().check()
    assert back.dtype == torch.float32 and torch.equal(back, x)
    half = m.decode_batch_async(lists, dev, tensor=dict(size=(32, 32), dtype=torch.float16, origin=([3, 35], [61, 0]), flip=[0, 1],
                                                        mean=IMAGENET[0], std=IMAGENET[1]))
    m.codec().check()
    assert torch.equal(half.cpu(), spec(torch, crops(torch, list(u8), (32, 32), ([3, 35], [61, 0]), [0, 1]), *IMAGENET, dtype=torch.float16))
    with pytest.raises(ValueError):
        m.decode_batch_async(lists, dev, tensor=dict(size=(H, W)), pixels="rgb")
    with pytest.raises(ValueError):
        m.decode_batch_async(lists, dev, tensor=dict(size=(H, W)), flat=True)
    with pytest.raises(ValueError):
        m.encode_batch_async(u8.to(dev), pixels="f32")                        # (uint8 is not float32)
    if container == "auto":
        sizes = [(150, 131), (96, 160)]                                        # (two sizes "auto" codes with one lane kind)
        u8s = [torch.from_numpy(make_image("smooth", h, w, 40 + i)) for i, (h, w) in enumerate(sizes)]
        lists = m.encode_batch_async([(u.float() / 255).to(dev) for u in u8s], pixels="f32").lists()
        assert lists == m.encode_batch_async([u.numpy() for u in u8s]).lists()
        origin = ([54, 0], [3, 32])
        back = m.decode_batch_async(lists, dev, tensor=dict(size=(96, 128), origin=origin))
        m.codec().check()
        assert torch.equal(back.cpu(), spec(torch, crops(torch, u8s, (96, 128), origin)))


# ------------------------------------------------------------------------------------------------ 12. the binding INTEGRATION.md shows
def test_integration_md_float_binding_runs(torch_mod):
    """INTEGRATION.md's ctypes binding of the two calls, executed as written (only the library path is substituted) in the namespace of its
    section-1 binding: the containers of the packaged uint8 path, and the tensor of the spec."""
    import os
    import re
    from conftest import ROOT
    from llicti_amd import _lib
    from llicti_amd.codec import container_to_bytestream_list
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    torch = torch_mod
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(.*?)```", md, re.S)
    binding = next(b for b in blocks if b.startswith("# graphs/models/llicti_hip_binding.py"))
    mine = next(b for b in blocks if "def decode_tensor_hip" in b and "def compress_f32_hip" in b)
    ns = {}
    exec(compile(binding.replace('C.CDLL("libllicti_hip.so")', f'C.CDLL({_lib.SO_PATH!r})'), "INTEGRATION.md#binding", "exec"), ns)
    exec(compile(mine, "INTEGRATION.md#float", "exec"), ns)
    torch.manual_seed(1337)
    model = LLICTI(default_config(container="xrans2")).to("cuda:0").eval()
    hip = ns["HipPath"](model, 0)
    sizes = [(72, 104), (97, 130), (64, 200)]
    u8s = [torch.from_numpy(make_image("smooth", h, w, 30 + i)) for i, (h, w) in enumerate(sizes)]
    cont, seg, ws = ns["compress_f32_hip"](hip.ctx, [(u.float() / 255).to("cuda:0") for u in u8s], 0x500 | 2)
    for b, u in enumerate(u8s):
        want, _ = model.compress(u[None].to("cuda:0"))
        assert container_to_bytestream_list(cont[b].cpu().numpy(), seg[b].cpu().numpy()) == want, b
    y0, x0, flip = [8, 33, 0], [40, 0, 136], [1, 0, 1]
    out = ns["decode_tensor_hip"](hip.ctx, cont, seg, [h for h, _ in sizes], [w for _, w in sizes], 0x500 | 2, ws, 64, y0, x0, flip, *IMAGENET)
    ns["_chk"](ns["_L"].llicti_check_status(hip.ctx, None))
    assert torch.equal(out.cpu(), spec(torch, crops(torch, u8s, (64, 64), (y0, x0), flip), *IMAGENET, dtype=torch.float16))
