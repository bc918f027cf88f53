"""Per-image reduce on the GPU (run with -m gpu on an MI355X): the five llicti_decode_images_*_rv calls take one reduce PER IMAGE -- image b stops
at its own level and is exactly what the scalar call at that value gives for it, while level l runs for the images with r_b <= l alone.  Every
comparison is EXACT; the yardsticks are the ORIGINAL pixels (rgb[:, ::2^r_b, ::2^r_b], which the decode side never sees) and tests/ref_resize.py,
never the scalar call alone.  Every decode runs on a workspace poisoned with 0xA5, and one case runs again on a context that has done nothing else.
Containers: xrans3, "auto", rans4 and wrans3 for config A; config B codes xwide streams only (xrans3, "auto")."""
import ctypes as C

import numpy as np
import pytest

import ref_resize as rr
from helpers import StreamGate, corruptions, make_image
from test_hip_reduced_decode import _dev, _encode, _new_codec, codecs, torch_mod  # noqa: F401  (the fixtures and the batch encoder)
from test_hip_resize import IMAGENET, assert_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = 0xA5
MIXED = [(67, 93), (64, 48), (33, 64), (150, 200), (96, 96), (67, 93)]
EQUAL = [(67, 93)] * 5
ALIGNED = [(64, 96)] * 4                       # W % 4 == 0, planes aligned: the sinks' 4-pixel path where r_b == 0
B_MIXED = [(67, 93), (32, 32), (64, 48)]
PATTERNS = {"mixed": [[0, 1, 2, 3, 5, 4], [5, 0, 5, 0, 5, 0], [1, 1, 0, 1, 1, 1], [2, 3, 2, 5, 4, 2]],      # (the last: no level-0 launch, no tail)
            "equal": [[0, 2, 1, 5, 0]], "aligned": [[0, 3, 1, 0]], "b": [[0, 2, 1]]}
SIZES = {"mixed": MIXED, "equal": EQUAL, "aligned": ALIGNED, "b": B_MIXED}
A_CONTAINERS = ["xrans3", "auto", "rans4", "wrans3"]
COUNTERS = ("plan_builds", "device_syncs", "device_allocs")

_BATCHES = {}


class Bt:
    pass


def batch(torch, c, which, name, wname):
    """One encoded batch, made once per (batch, container, weights): the originals on the host, the containers on the device."""
    key = (which, name, wname)
    if key not in _BATCHES:
        bt = Bt()
        bt.sizes = SIZES[which]
        bt.rgbs = [make_image(("noise", "smooth")[i % 2], h, w, 500 + 7 * i + h) for i, (h, w) in enumerate(bt.sizes)]
        bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode = _encode(torch, c, bt.rgbs, name)
        bt.B = len(bt.sizes)
        _BATCHES[key] = bt
    return _BATCHES[key]


def subs(bt, rv):
    return [rgb[:, ::1 << r, ::1 << r] for rgb, r in zip(bt.rgbs, rv)]


def planar(c, bt, rv, **kw):
    """decode_reduced(reduce=[...]) on a poisoned workspace -> the flat host bytes; every status word is 0"""
    c.workspace_v(bt.Hs, bt.Ws, bt.mode)
    c.poison_workspace(POISON)
    flat = c.decode_reduced(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, rv, **kw)
    c.check()
    st = c.image_status(bt.B)
    assert (st == 0).all(), (rv, st)
    return flat.cpu().numpy()


def assert_planar(bt, host, rv, offs=None, what=""):
    pos = 0
    for b, want in enumerate(subs(bt, rv)):
        if offs is not None:
            pos = int(offs[b])
        got = host[pos:pos + want.size].reshape(want.shape)
        assert np.array_equal(got, want), (what, rv, "image", b, "differs from the original's [::2^%d]" % rv[b])
        pos += want.size
    return pos


# ------------------------------------------------------------------------------------------------ 1. planar
@pytest.mark.parametrize("wname", ["rand1337", "trainedlike"])
@pytest.mark.parametrize("name", A_CONTAINERS)
@pytest.mark.parametrize("which", ["mixed", "equal", "aligned"])
def test_planar_config_a(torch_mod, codecs, which, name, wname):
    torch = torch_mod
    c = codecs(wname)
    bt = batch(torch, c, which, name, wname)
    for rv in PATTERNS[which]:
        host = planar(c, bt, rv)
        assert assert_planar(bt, host, rv, what=(which, name, wname)) == host.size      # tight, each image at its own reduced size


@pytest.mark.parametrize("wname", ["rand1337", "trainedlike"])
@pytest.mark.parametrize("name", ["xrans3", "auto"])
def test_planar_config_b(torch_mod, codecs, name, wname):
    torch = torch_mod
    c = codecs(wname, 2)
    bt = batch(torch, c, "b", name, "b_" + wname)
    for rv in PATTERNS["b"] + [[2, 0, 2], [1, 2, 1]]:
        host = planar(c, bt, rv)
        assert assert_planar(bt, host, rv, what=("b", name, wname)) == host.size


def test_planar_on_a_fresh_context_and_with_caller_offsets(torch_mod, codecs):
    """The first call a context ever makes is a per-image one (nothing cached, no block pooled); then rgb_off: the images at caller-chosen,
    unordered, non-tight offsets, every byte outside them kept."""
    torch = torch_mod
    bt = batch(torch, codecs("trainedlike"), "mixed", "xrans3", "trainedlike")
    fresh = _new_codec("trainedlike", 5)
    try:
        for rv in PATTERNS["mixed"][:2]:
            assert_planar(bt, planar(fresh, bt, rv), rv, what="fresh")
        rv = PATTERNS["mixed"][0]
        n = [s.size for s in subs(bt, rv)]
        order = [3, 0, 5, 1, 4, 2]
        offs, pos = np.zeros(bt.B, dtype=np.uint64), 5
        for b in order:
            offs[b] = pos
            pos += n[b] + 3 + 2 * b
        out = torch.full((pos + 9,), 0x3C, dtype=torch.uint8, device=DEV)
        host = planar(fresh, bt, rv, rgb_off=offs, out=out)
        assert_planar(bt, host, rv, offs=offs, what="rgb_off")
        covered = np.zeros(host.size, dtype=bool)
        for b in range(bt.B):
            covered[int(offs[b]):int(offs[b]) + n[b]] = True
        assert (host[~covered] == 0x3C).all()
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ 2. interleaved pixels
@pytest.mark.parametrize("fmt", ["rgb", "bgr", "rgba", "bgra"])
@pytest.mark.parametrize("which,name", [("mixed", "xrans3"), ("aligned", "auto"), ("mixed", "wrans3"), ("equal", "rans4")])
def test_px_into_a_pitched_canvas(torch_mod, codecs, which, name, fmt):
    """Every image's window in one canvas, rows a pitch apart, the first window at an odd byte (the aligned batch: at a multiple of 4 with pitches
    that are, so that the dword stores and the short4 loads run where r_b == 0): the windows hold the originals' subsamples in the format's byte
    order, alpha 255, and every other byte of the canvas is kept."""
    torch = torch_mod
    c = codecs("trainedlike")
    bt = batch(torch, c, which, name, "trainedlike")
    bpp = 4 if fmt.endswith("a") else 3
    for rv in PATTERNS[which]:
        want = subs(bt, rv)
        al = which == "aligned"
        pitch, offs, pos = [], [], (8 if al else 7)
        for b, s in enumerate(want):
            pt = s.shape[2] * bpp + (8 if al else 5 + b)
            pt += (-pt) % 4 if al else 0
            pitch.append(pt)
            offs.append(pos)
            pos += s.shape[1] * pt + (4 if al else 3)
        canvas = torch.full((pos + 11,), 0x5E, dtype=torch.uint8, device=DEV)
        c.workspace_v(bt.Hs, bt.Ws, bt.mode)
        c.poison_workspace(POISON)
        out = c.decode_px(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, fmt, reduce=rv, out=canvas, px_off=offs, pitch=pitch)
        c.check()
        assert (c.image_status(bt.B) == 0).all() and out.data_ptr() == canvas.data_ptr()
        host = canvas.cpu().numpy()
        covered = np.zeros(host.size, dtype=bool)
        for b, s in enumerate(want):
            h, w = s.shape[1:]
            idx = offs[b] + np.arange(h)[:, None] * pitch[b] + np.arange(w * bpp)[None, :]
            win = host[idx].reshape(h, w, bpp)
            px = s.transpose(1, 2, 0)
            assert np.array_equal(win[..., :3], px[..., ::-1] if fmt.startswith("bgr") else px), (which, name, fmt, rv, b)
            if bpp == 4:
                assert (win[..., 3] == 255).all()
            covered[idx] = True
        assert (host[~covered] == 0x5E).all(), (which, name, fmt, rv, "bytes outside the windows changed")


# ------------------------------------------------------------------------------------------------ 3. float tensors
def _dt(torch, name):
    return getattr(torch, name)


@pytest.mark.parametrize("dt", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("which,name", [("mixed", "xrans3"), ("aligned", "rans4"), ("equal", "auto")])
def test_tensor_windows(torch_mod, codecs, which, name, dt):
    """decode_tensor(reduce=[...]): an Ho x Wo window per image at an origin of ITS OWN decimated grid, some mirrored, normalised -- against
    ref_resize.finish on the original's subsample; and nothing is written outside the tensor."""
    torch = torch_mod
    c = codecs("trainedlike")
    bt = batch(torch, c, which, name, "trainedlike")
    tdt = _dt(torch, dt)
    es = torch.empty((), dtype=tdt).element_size()
    for k, rv in enumerate(PATTERNS[which]):
        want_imgs = subs(bt, rv)
        Ho, Wo = min([4] + [s.shape[1] for s in want_imgs]), min([8] + [s.shape[2] for s in want_imgs])      # (33 x 64 at r = 5 is 2 x 2; 64 x 96 at r = 3 is 8 x 12)
        y0 = [(s.shape[1] - Ho) // (1 + b % 2) for b, s in enumerate(want_imgs)]
        x0 = [((s.shape[2] - Wo) // (1 + (b + 1) % 2)) & (~3 if which == "aligned" else ~0) for b, s in enumerate(want_imgs)]
        flip = [int((b + k) % 3 == 0) for b in range(bt.B)]
        if which == "aligned":
            flip = [0] * bt.B                                    # (unflipped, x0 % 4 == 0: the short4 path for the images at r = 0)
        nb, pad = bt.B * 3 * Ho * Wo * es, 64
        big = torch.full((pad + nb + 64,), POISON, dtype=torch.uint8, device=DEV)
        out = big[pad:pad + nb].view(tdt).view(bt.B, 3, Ho, Wo)
        c.workspace_v(bt.Hs, bt.Ws, bt.mode)
        c.poison_workspace(POISON)
        got = c.decode_tensor(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, (Ho, Wo), dtype=tdt, origin=(y0, x0), flip=flip, mean=IMAGENET[0], std=IMAGENET[1],
                              reduce=rv, out=out)
        c.check()
        assert (c.image_status(bt.B) == 0).all() and got.data_ptr() == out.data_ptr()
        want = []
        for b, s in enumerate(want_imgs):
            v = rr.finish(s[:, y0[b]:y0[b] + Ho, x0[b]:x0[b] + Wo].astype(np.float32), IMAGENET[0], IMAGENET[1], dt)
            want.append(v[:, :, ::-1] if flip[b] else v)
        assert_bits(torch, got, np.stack(want), (which, name, dt, rv))
        host = big.cpu()
        assert (host[:pad] == POISON).all() and (host[pad + nb:] == POISON).all()


def _boxes_for(want_imgs, size, k, antialias):
    """a box per image on its own decimated grid: whole images, interior boxes and boxes ending at the last row and column by turns; with the
    filter a box shrinks by at most 4"""
    boxes = []
    for b, s in enumerate(want_imgs):
        H, W = s.shape[1:]
        hs, ws = (H, W) if (b + k) % 3 == 0 else (max(1, H - 1 - b % 2), max(1, W - 2))
        if antialias:
            hs, ws = min(hs, 4 * size[0]), min(ws, 4 * size[1])
        y0, x0 = ((H - hs), (W - ws)) if (b + k) % 3 == 1 else ((H - hs) // 2, (W - ws) // 2)
        boxes.append((y0, x0, hs, ws))
    return boxes


@pytest.mark.parametrize("dt", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("antialias", [0, 1])
@pytest.mark.parametrize("which,name", [("mixed", "xrans3"), ("equal", "wrans3"), ("aligned", "auto")])
def test_resized_crops(torch_mod, codecs, which, name, antialias, dt):
    """decode_tensor_resized(reduce=[...]): a box per image in the coordinates of its own grid, resampled to one size -- bit for bit
    ref_resize.resized_crop on the original's subsample -- inside guard bands."""
    torch = torch_mod
    c = codecs("rand1337")
    bt = batch(torch, c, which, name, "rand1337")
    tdt = _dt(torch, dt)
    es = torch.empty((), dtype=tdt).element_size()
    size = (7, 10)
    for k, rv in enumerate(PATTERNS[which]):
        want_imgs = subs(bt, rv)
        boxes = _boxes_for(want_imgs, size, k, antialias)
        flip = [int((b + k) % 2) for b in range(bt.B)]
        nb, pad = bt.B * 3 * size[0] * size[1] * es, es               # (one element in: element stores)
        big = torch.full((pad + nb + 64,), POISON, dtype=torch.uint8, device=DEV)
        out = big[pad:pad + nb].view(tdt).view(bt.B, 3, *size)
        c.workspace_v(bt.Hs, bt.Ws, bt.mode)
        c.poison_workspace(POISON)
        got = c.decode_tensor_resized(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size, boxes, dtype=tdt, flip=flip, mean=IMAGENET[0], std=IMAGENET[1],
                                      antialias=bool(antialias), reduce=rv, out=out)
        c.check()
        assert (c.image_status(bt.B) == 0).all()
        want = np.stack([rr.resized_crop(s, box, size, antialias, bool(f), IMAGENET[0], IMAGENET[1], dt) for s, box, f in zip(want_imgs, boxes, flip)])
        assert_bits(torch, got, want, (which, name, antialias, dt, rv))
        host = big.cpu()
        assert (host[:pad] == POISON).all() and (host[pad + nb:] == POISON).all()


@pytest.mark.parametrize("dt", ["float32", "float16", "bfloat16"])
def test_views_two_groups_and_an_image_no_view_names(torch_mod, codecs, dt):
    """decode_tensor_views(reduce=[...]): two groups of different size, views in scrambled order with repeats; image 4 is named by no view and
    passed at the model's level count.  Every view is ref_resize.resized_crop on ITS image's subsample; guard bands around both tensors."""
    torch = torch_mod
    c = codecs("trainedlike")
    bt = batch(torch, c, "mixed", "xrans3", "trainedlike")
    tdt = _dt(torch, dt)
    for rv in ([0, 1, 2, 3, 5, 4], [2, 0, 1, 0, 5, 3]):
        want_imgs = subs(bt, rv)
        specs = [dict(size=(6, 9), image=[3, 0, 5, 3, 1, 2, 0], flip=[1, 0, 0, 1, 0, 1, 1], antialias=True, dtype=tdt),
                 dict(size=(3, 4), image=[5, 5, 2, 0], flip=None, antialias=False, dtype=torch.float32)]
        groups, bigs = [], []
        for g in specs:
            boxes = []
            for v, b in enumerate(g["image"]):
                H, W = want_imgs[b].shape[1:]
                hs, ws = max(1, H - v % 3), max(1, W - (v + 1) % 3)
                if g["antialias"]:
                    hs, ws = min(hs, 4 * g["size"][0]), min(ws, 4 * g["size"][1])
                boxes.append(((H - hs) // (1 + v % 2), (W - ws) // (1 + (v + 1) % 2), hs, ws))
            es = torch.empty((), dtype=g["dtype"]).element_size()
            nb, pad = len(boxes) * 3 * g["size"][0] * g["size"][1] * es, 64
            big = torch.full((pad + nb + 64,), POISON, dtype=torch.uint8, device=DEV)
            bigs.append((big, pad, nb))
            groups.append(dict(g, boxes=boxes, out=big[pad:pad + nb].view(g["dtype"]).view(-1, 3, *g["size"])))
        c.workspace_v(bt.Hs, bt.Ws, bt.mode)
        c.poison_workspace(POISON)
        outs = c.decode_tensor_views(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, groups, mean=IMAGENET[0], std=IMAGENET[1], reduce=rv)
        c.check()
        assert (c.image_status(bt.B) == 0).all()
        for g, out, (big, pad, nb) in zip(groups, outs, bigs):
            name = {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}[g["dtype"]]
            fl = g["flip"] or [0] * len(g["image"])
            want = np.stack([rr.resized_crop(want_imgs[b], box, g["size"], int(g["antialias"]), bool(f), IMAGENET[0], IMAGENET[1], name)
                             for b, box, f in zip(g["image"], g["boxes"], fl)])
            assert_bits(torch, out, want, (dt, rv, g["size"]))
            host = big.cpu()
            assert (host[:pad] == POISON).all() and (host[pad + nb:] == POISON).all()


# ------------------------------------------------------------------------------------------------ 4. the work is skipped
@pytest.mark.parametrize("name", ["xrans3", "rans4"])
def test_skipped_levels_are_neither_decoded_nor_launched(torch_mod, codecs, name):
    """The equal-size batch: after the call, every plane sample of image b OFF its 2^r_b grid still holds the poison, every sample ON it the
    lifted original (YCoCg-R in numpy); the call reports 3 (nlev - min r) band-CNN launches, none when every image is at nlev."""
    torch = torch_mod
    c = codecs("trainedlike")
    bt = batch(torch, c, "equal", name, "trainedlike")
    H, W = EQUAL[0]
    o16, o32 = C.c_size_t(), C.c_size_t()
    from llicti_amd import _lib
    _lib.check(c.L.llicti_workspace_planes(c.ctx, bt.B, H, W, bt.mode, C.byref(o16), C.byref(o32)))
    c.set_profiling(True)
    try:
        for rv in ([0, 2, 1, 5, 0], [3, 2, 4, 5, 2], [5, 5, 4, 5, 5]):
            host = planar(c, bt, rv)
            assert_planar(bt, host, rv)
            assert c.last_timing()[1] == 3 * (5 - min(rv)), (rv, c.last_timing())
            lev = c.last_cnn_level_ms()
            assert all(v == 0 for v in lev[:min(rv)]) and all(v > 0 for v in lev[min(rv):5]), (rv, lev)
            cat = c.last_timing_detail()[0]
            assert (cat["rans_tail"] > 0) == (min(rv) == 0), (rv, cat)
            planes = c._ws[o16.value:o16.value + bt.B * 3 * H * W * 2].view(torch.int16).view(bt.B, 3, H, W).cpu().numpy()
            for b, (rgb, r) in enumerate(zip(bt.rgbs, rv)):
                R, G, Bl = (rgb[k].astype(np.int32) for k in range(3))
                Co = R - Bl
                t = Bl + (Co >> 1)
                Cg = G - t
                lifted = np.stack([t + (Cg >> 1) - 127, Co, Cg]).astype(np.int16)
                on = np.zeros((H, W), dtype=bool)
                on[::1 << r, ::1 << r] = True
                assert np.array_equal(planes[b][:, on], lifted[:, on]), (rv, b, "a sample on the image's grid is not the lifted original")
                assert (planes[b][:, ~on].view(np.uint16) == 0xA5A5).all(), (rv, b, "a sample off the image's 2^r grid was written")
        host = planar(c, bt, [5] * 5)                           # all equal: the scalar call, which launches no CNN at nlev
        assert_planar(bt, host, [5] * 5)
        assert c.last_timing()[1] == 0
    finally:
        c.set_profiling(False)


# ------------------------------------------------------------------------------------------------ 5. status
def test_a_damaged_container_reports_what_the_scalar_call_reports(torch_mod, codecs):
    """A single flipped bit in the initial states of image 2's stream 0, one the full decode flags: at r_2 = 0 the per-image call gives image 2
    the scalar full decode's word and its neighbours 0 (and their pixels); moved to an image with r = nlev it gives what the scalar call at
    reduce = nlev reports for it."""
    torch = torch_mod
    from llicti_amd._lib import EFORMAT, LlictiError
    from llicti_amd.codec import container_to_bytestream_list
    c = codecs("rand1337")
    bt = batch(torch, c, "mixed", "xrans3", "rand1337")
    seg_h = bt.seg.cpu().numpy()

    def damaged(b, bit):
        bad = bt.cont.clone()
        bad[b, int(seg_h[b, :4].sum()) + (bit >> 3)] ^= 1 << (bit & 7)
        return bad

    def words(cont, reduce):
        c.workspace_v(bt.Hs, bt.Ws, bt.mode)
        c.poison_workspace(POISON)
        flat = c.decode_reduced(cont, bt.seg, bt.Hs, bt.Ws, bt.mode, reduce)
        try:
            c.check()
        except LlictiError as e:
            assert e.code == EFORMAT, e
        return list(c.image_status(bt.B)), flat.cpu().numpy()

    def flagged_flip(b):
        bl = container_to_bytestream_list(bt.cont[b].cpu().numpy(), seg_h[b])
        for kind, bit in [f for f in corruptions(bl[1][0], 256, "v4", seed=11) if f[0] == "state"][:8]:
            st, _ = words(damaged(b, bit), 0)
            if st[b] != 0:
                assert all(v == 0 for k, v in enumerate(st) if k != b)
                return bit, st[b]
        raise AssertionError("none of the first eight state flips is flagged by the full decode")

    rv = [1, 3, 0, 2, 5, 0]
    bit, word = flagged_flip(2)
    st, host = words(damaged(2, bit), rv)
    assert st == [0, 0, word, 0, 0, 0], st
    pos = 0
    for b, want in enumerate(subs(bt, rv)):
        if b != 2:
            assert np.array_equal(host[pos:pos + want.size].reshape(want.shape), want), b
        pos += want.size
    # the same kind of damage at the image that stops at nlev: the scalar call at reduce = nlev is the yardstick
    bit4, _ = flagged_flip(4)
    st_scalar, _ = words(damaged(4, bit4), 5)
    st_rv, _ = words(damaged(4, bit4), rv)
    assert st_rv[4] == st_scalar[4] and all(v == 0 for k, v in enumerate(st_rv) if k != 4), (st_rv, st_scalar)
    c.check()


# ------------------------------------------------------------------------------------------------ 6. all equal, and the host's cost
@pytest.mark.parametrize("name", ["xrans3", "ac"])
def test_all_equal_is_the_scalar_call(torch_mod, codecs, name):
    """reduce = [r] * B: the bytes of reduce = r (the reference format included), and no plan is built when the scalar call ran first."""
    torch = torch_mod
    c = codecs("trainedlike")
    bt = batch(torch, c, "equal", name, "trainedlike")
    for r in (0, 2, 5):
        c.workspace_v(bt.Hs, bt.Ws, bt.mode)
        c.poison_workspace(POISON)
        a = c.decode_reduced(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, r).clone()
        c.check()
        before = {k: c.counter(k) for k in COUNTERS}
        c.poison_workspace(POISON)
        b = c.decode_reduced(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, [r] * bt.B)
        c.check()
        assert torch.equal(a, b) and {k: c.counter(k) for k in COUNTERS} == before, (name, r)
        assert_planar(bt, b.cpu().numpy(), [r] * bt.B)
        size, boxes = (5, 7), [(0, 0, *s.shape[1:]) for s in subs(bt, [r] * bt.B)]
        t0 = c.decode_tensor_resized(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size, boxes, antialias=False, reduce=r).clone()
        t1 = c.decode_tensor_resized(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size, boxes, antialias=False, reduce=[r] * bt.B)
        c.check()
        assert torch.equal(t0, t1)


def test_fresh_reduces_and_boxes_every_call_cost_nothing_on_the_host(torch_mod, codecs):
    """Twelve calls with new reduces, boxes and flips each (after two of warm-up): no plan is built, the device is neither synchronised by the
    library nor asked for memory -- the per-call tables come from the pool -- and every result is exact."""
    torch = torch_mod
    c = codecs("trainedlike")
    bt = batch(torch, c, "mixed", "xrans3", "trainedlike")
    rng = np.random.default_rng(77)
    size = (6, 8)
    before, calls = None, []
    for it in range(14):
        if it == 2:
            before = {k: c.counter(k) for k in COUNTERS}
        rv = [int(v) for v in rng.integers(0, 6, bt.B)]
        if len(set(rv)) == 1:
            rv[0] = (rv[0] + 1) % 6
        boxes = []
        for s in subs(bt, rv):
            H, W = s.shape[1:]
            hs, ws = int(rng.integers(1, min(H, 4 * size[0]) + 1)), int(rng.integers(1, min(W, 4 * size[1]) + 1))
            boxes.append((int(rng.integers(0, H - hs + 1)), int(rng.integers(0, W - ws + 1)), hs, ws))
        flip = [int(v) for v in rng.integers(0, 2, bt.B)]
        c.poison_workspace(POISON)
        out = c.decode_tensor_resized(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size, boxes, flip=flip, reduce=rv)
        c.check()
        calls.append((rv, boxes, flip, out))
    assert {k: c.counter(k) for k in COUNTERS} == before
    for rv, boxes, flip, out in calls:
        want = np.stack([rr.resized_crop(s, box, size, 1, bool(f)) for s, box, f in zip(subs(bt, rv), boxes, flip)])
        assert_bits(torch, out, want, rv)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_are_einval_name_the_image_and_launch_nothing(torch_mod, codecs):
    torch = torch_mod
    from llicti_amd._lib import EINVAL, LlictiError
    from llicti_amd.codec import _ptr, _stream_ptr
    c = codecs("trainedlike")
    bt = batch(torch, c, "mixed", "xrans3", "trainedlike")
    ac = batch(torch, c, "equal", "ac", "trainedlike")
    good = [0, 1, 2, 3, 5, 4]
    assert_planar(bt, planar(c, bt, good), good)                 # (warm; the status words are clean)
    n = sum(s.size for s in bt.rgbs)                              # (room for every image at full size: the wrapper sizes a refused value as 0)
    out = torch.full((n,), 0x77, dtype=torch.uint8, device=DEV)
    tout = torch.full((bt.B, 3, 4, 4), float("nan"), device=DEV)
    before = {k: c.counter(k) for k in COUNTERS + ("plan_hits",)}
    dims = [s.shape[1:] for s in subs(bt, good)]

    def refused(words, fn):
        with pytest.raises(LlictiError) as e:
            fn()
        assert e.value.code == EINVAL and all(w in str(e.value) for w in words), (words, str(e.value))

    # a value out of range, naming the image
    refused(("image 3", "6"), lambda: c.decode_reduced(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, [0, 1, 2, 6, 5, 4], out=out))
    refused(("image 1", "-1"), lambda: c.decode_px(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, "rgb", reduce=[0, -1, 2, 3, 5, 4]))
    refused(("image 5",), lambda: c.decode_tensor(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, (1, 1), reduce=[0, 1, 2, 3, 5, 7], out=tout))
    # differing values with a reference-format container in the call
    refused(("image 1", "reference-format"), lambda: c.decode_reduced(ac.cont, ac.seg, ac.Hs, ac.Ws, ac.mode, [0, 2, 1, 5, 0]))
    refused(("image 2", "reference-format"), lambda: c.decode_tensor_resized(ac.cont, ac.seg, ac.Hs, ac.Ws, ac.mode, (4, 4), None, antialias=False, reduce=[1, 1, 0, 1, 1]))
    # what the sibling refuses at THAT image's reduce: a window / box that fits image 4 at r = 4 but not at its r = 5 (3 x 3)
    refused(("image 4", "leaves"), lambda: c.decode_tensor(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, (4, 4), reduce=good, out=tout))
    boxes = [(0, 0, h, w) for h, w in dims]
    boxes[2] = (0, 0, dims[2][0] + 1, dims[2][1])                # one row more than image 2 has at ITS r = 2
    refused(("image 2", "leaves"), lambda: c.decode_tensor_resized(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, (4, 4), boxes, antialias=False, reduce=good))
    boxes[2] = (0, 0, *dims[2])
    refused(("image 0", "raise reduce"), lambda: c.decode_tensor_resized(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, (4, 4), boxes, antialias=True, reduce=good))
    g = dict(size=(2, 2), image=[1, 4], boxes=[(0, 0, *dims[1]), (0, 0, 4, 3)], antialias=False)      # image 4 at r = 5 has 3 rows
    refused(("view 1", "image 4", "leaves"), lambda: c.decode_tensor_views(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, [g], reduce=good))
    with pytest.raises(ValueError):
        c.decode_reduced(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, [0, 1, 2])      # (not one per image: the wrapper's own refusal)
    # a null array: only the C call can say that
    Hs, Ws = np.asarray(bt.Hs, dtype=np.int32), np.asarray(bt.Ws, dtype=np.int32)
    ws = c.workspace_v(Hs, Ws, bt.mode)
    modes = np.array([bt.mode], dtype=np.int32)
    rc = c.L.llicti_decode_images_reduced_rv(c.ctx, _ptr(bt.cont), bt.cont.shape[1], _ptr(bt.seg), bt.B, _ptr(Hs), _ptr(Ws), _ptr(modes), 1, None,
                                             _ptr(ws), ws.numel(), _ptr(out), None, _stream_ptr(c.device))
    assert rc == EINVAL and "null reduces" in c.L.llicti_last_error().decode()
    assert {k: c.counter(k) for k in before} == before           # no plan was looked up, built or uploaded
    assert (out == 0x77).all() and torch.isnan(tout).all()       # nothing was written ...
    c.check()
    assert (c.image_status(bt.B) == 0).all()                     # ... and the words are the last good call's


# ------------------------------------------------------------------------------------------------ 8. ordering
def test_on_a_callers_stream_behind_a_gate(torch_mod, codecs):
    """The call on a caller's stream that a gate (helpers.StreamGate) holds busy: the containers it reads are DECOYS until a copy, enqueued on
    that stream behind the gate, overwrites them.  Everything is enqueued before the gate ends (asserted), so a launch -- or the upload of the
    call's own tables, made fresh for THIS call's reduces -- that was not ordered on the stream would have worked on the wrong data."""
    torch = torch_mod
    c = codecs("trainedlike")
    bt = batch(torch, c, "mixed", "xrans3", "trainedlike")
    decoy_rgbs = [make_image(("smooth", "noise")[i % 2], h, w, 900 + i) for i, (h, w) in enumerate(MIXED)]
    dcont, dseg, _, _, dmode = _encode(torch, c, decoy_rgbs, "xrans3")
    assert dmode == bt.mode and dcont.shape == bt.cont.shape and not torch.equal(dcont, bt.cont)
    warm, rv = [5, 4, 3, 2, 1, 0], [0, 1, 2, 3, 5, 4]             # (the warm-up's tables are NOT this call's)
    s = torch.cuda.Stream(device=DEV)
    gate = StreamGate(torch, DEV)
    with torch.cuda.stream(s):
        c.workspace_v(bt.Hs, bt.Ws, bt.mode)
        c.decode_reduced(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, warm)
        c.check()
    torch.cuda.synchronize()
    cont, seg = dcont.clone(), dseg.clone()
    n = sum(x.size for x in subs(bt, rv))
    out = torch.full((n,), 0x11, dtype=torch.uint8, device=DEV)
    c.poison_workspace(POISON)
    torch.cuda.synchronize()
    begin, end = gate.hold(s, 100.0)
    with torch.cuda.stream(s):
        cont.copy_(bt.cont, non_blocking=True)
        seg.copy_(bt.seg, non_blocking=True)
        c.decode_reduced(cont, seg, bt.Hs, bt.Ws, bt.mode, rv, out=out)
        got = torch.empty_like(out)
        got.copy_(out, non_blocking=True)
    assert not end.query(), "the gate ended before the last enqueue: the run proves nothing"
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c.check()
        assert (c.image_status(bt.B) == 0).all()
    assert_planar(bt, got.cpu().numpy(), rv, what="gated")


# ------------------------------------------------------------------------------------------------ 9. the model layer
def test_model_layer_takes_a_reduce_per_image(torch_mod):
    """LLICTI.decode_batch_async(lists, reduce=[...], tensor=dict(views=...)) with multi_crop_plan(per_image=True)'s reduces and boxes, and
    decompres_batch(reduce=[...]): a list, image b at its own reduced size."""
    torch = torch_mod
    from llicti_amd.codec import multi_crop_plan
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    torch.manual_seed(1337)
    m = LLICTI(default_config(container="xrans2")).to(DEV).eval()
    dev = torch.device(DEV)
    sizes = [(150, 131), (96, 160), (67, 93)]
    rgbs = [make_image("smooth", h, w, 40 + i) for i, (h, w) in enumerate(sizes)]
    lists = m.encode_batch_async(rgbs).lists()
    full = [((32, 28), [0, 1, 1], [(3, 8, 140, 120), (0, 20, 96, 130), (10, 0, 80, 70)]), ((12, 12), [1, 0], [(40, 50, 30, 30), (100, 90, 50, 41)])]
    rs, boxes = multi_crop_plan(sizes, full, per_image=True)
    assert rs == [1, 1, 5]                                         # (image 2 is named by no view: the model's level count)
    rs1, boxes1 = multi_crop_plan(sizes[:2], full)
    assert rs1 == 1 and boxes == boxes1                            # both images' tightest views allow r = 1: the scalar plan's boxes
    full2 = [((32, 28), [0, 1], [(3, 8, 140, 120), (0, 20, 96, 130)]), ((12, 12), [1, 2], [(40, 50, 30, 30), (10, 20, 50, 41)])]
    rs, boxes = multi_crop_plan(sizes, full2, per_image=True)
    assert rs == [2, 1, 1] and boxes[0][0] == (1, 2, 35, 30) and boxes[1] == [(20, 25, 15, 15), (5, 10, 25, 21)]      # (41 columns keep 11 < 12 at r = 2)
    groups = [dict(size=(32, 28), image=[0, 1], boxes=boxes[0], flip=[1, 0], dtype=torch.float16), dict(size=(12, 12), image=[1, 2], boxes=boxes[1])]
    m.codec().poison_workspace()
    got = m.decode_batch_async(lists, dev, reduce=rs, tensor=dict(views=groups, mean=IMAGENET[0], std=IMAGENET[1]))
    m.codec().check()
    assert isinstance(got, list) and len(got) == 2
    for g, out in zip(groups, got):
        name = "float16" if g.get("dtype") == torch.float16 else "float32"
        want = np.stack([rr.resized_crop(rgbs[b][:, ::1 << rs[b], ::1 << rs[b]], box, g["size"], 1, bool(f), *IMAGENET, name)
                         for b, box, f in zip(g["image"], g["boxes"], g.get("flip") or [0, 0])])
        assert_bits(torch, out, want, g["size"])
    m.codec().poison_workspace()
    outs = m.decompres_batch(lists, dev, reduce=[0, 3, 1])
    assert isinstance(outs, list) and [tuple(o.shape) for o in outs] == [(1, 3, 150, 131), (1, 3, 12, 20), (1, 3, 34, 47)]
    for o, rgb, r in zip(outs, rgbs, [0, 3, 1]):
        assert torch.equal(o, (_dev(torch, rgb[:, ::1 << r, ::1 << r]).to(torch.float32) / 255)[None])
    flat, Hs, Ws = m.decode_batch_async(lists, dev, reduce=[2, 0, 5])
    m.codec().check()
    assert (Hs, Ws) == ([38, 96, 3], [33, 160, 3]) and flat.numel() == 3 * (38 * 33 + 96 * 160 + 9)
    with pytest.raises(ValueError):
        m.decode_batch_async(lists, dev, reduce=[0, 1])
