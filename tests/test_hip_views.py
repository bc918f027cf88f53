"""Views on the GPU (run with -m gpu on an MI355X): llicti_decode_images_tensor_views decodes a batch ONCE and writes several resized crops per
image, in groups of one output size each.  Every check is EXACT (bit for bit), against two references that are independent of the code under
test: tests/ref_resize.resized_crop on the image decode_v returns, and the existing decode_tensor_resized on the containers gathered with
containers[image].  Images: helpers.make_image at 33x47, 64x96 and 96x67 in one xrans2 call, built as tests/test_hip_resize.py builds its mixed
batch; every decode runs on a poisoned workspace."""
import ctypes as C

import numpy as np
import pytest

import ref_resize as rr
from helpers import StreamGate
from test_hip_resize import DEV, IMAGENET, POISON, assert_bits, batch, codec, tname, torch_mod  # noqa: F401  (the fixtures and the batch builder)

pytestmark = pytest.mark.gpu

SIZES = [(33, 47), (64, 96), (96, 67)]
SEED = 700
# test 1 -- group 0: seven views of three images in no order, to (16, 24) with the filter (every box at most 64 x 96): a whole image (33 x 47), a
# whole image at a scale of exactly 4 (64 x 96), a magnified box (9 x 11), a one-pixel-wide box, and boxes ending at the last row and column
G0 = dict(size=(16, 24), image=[2, 0, 0, 1, 2, 2, 0], flip=[1, 0, 1, 0, 0, 1, 0], antialias=True,
          boxes=[(10, 3, 64, 60), (0, 0, 33, 47), (5, 7, 9, 11), (0, 0, 64, 96), (0, 30, 50, 1), (32, 7, 64, 60), (1, 1, 31, 45)])
# group 1: five views of image 1 alone, to (13, 19) without the filter: the whole image, a magnified box, a one-pixel-wide and a one-pixel-high one
G1 = dict(size=(13, 19), image=[1, 1, 1, 1, 1], flip=None, antialias=False,
          boxes=[(0, 0, 64, 96), (3, 5, 6, 8), (10, 95, 40, 1), (63, 0, 1, 96), (7, 9, 50, 70)])


def mixed(torch, c):
    return batch(torch, c, SIZES, seed=SEED)


_DECODED = {}


def decoded(torch, c, bt):
    """The images decode_v returns for the batch, on the host, made once (they are the original pixels: the codec is lossless)"""
    if id(bt) not in _DECODED:
        c.poison_workspace(POISON)
        flat = c.decode_v(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode)
        c.check()
        flat = flat.cpu().numpy()
        imgs, off = [], 0
        for (h, w), rgb in zip(bt.sizes, bt.rgbs):
            imgs.append(flat[off:off + 3 * h * w].reshape(3, h, w).copy())
            off += 3 * h * w
            assert np.array_equal(imgs[-1], rgb)
        _DECODED[id(bt)] = imgs
    return _DECODED[id(bt)]


def n_views(bt, g):
    return len(bt.sizes) if g.get("image") is None else len(g["image"])


def whole_boxes(bt, g, reduce):
    from llicti_amd.codec import reduced_dims
    image = g.get("image") or range(len(bt.sizes))
    return [(0, 0) + tuple(reduced_dims(*bt.sizes[b], reduce)) for b in image]


def ref_numpy(torch, c, bt, g, mean=None, std=None, reduce=0):
    """reference 1: ref_resize.resized_crop per view, on the decoded image of the view's index (decimated by 2^reduce)"""
    imgs = decoded(torch, c, bt)
    image = g.get("image") or list(range(len(bt.sizes)))
    boxes = g.get("boxes") or whole_boxes(bt, g, reduce)
    flip = g.get("flip") or [0] * len(image)
    dt = tname(torch, g.get("dtype", torch.float32))
    s = 1 << reduce
    return np.stack([rr.resized_crop(imgs[b][:, ::s, ::s], box, g["size"], int(g.get("antialias", True)), bool(f), mean, std, dt)
                     for b, box, f in zip(image, boxes, flip)])


def ref_resized(torch, c, bt, g, mean=None, std=None, reduce=0):
    """reference 2: the existing decode_tensor_resized on the containers gathered with containers[image] -- one whole decode per view"""
    image = g.get("image") or list(range(len(bt.sizes)))
    idx = torch.as_tensor(image, device=DEV, dtype=torch.long)
    c.poison_workspace(POISON)
    out = c.decode_tensor_resized(bt.cont[idx].contiguous(), bt.seg[idx].contiguous(), [bt.Hs[b] for b in image], [bt.Ws[b] for b in image], bt.mode,
                                  g["size"], g.get("boxes"), dtype=g.get("dtype", torch.float32), flip=g.get("flip"), mean=mean, std=std,
                                  antialias=g.get("antialias", True), reduce=reduce)
    c.check()
    return out


def views(c, bt, groups, **kw):
    c.poison_workspace(POISON)
    outs = c.decode_tensor_views(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, groups, **kw)
    c.check()
    assert (c.image_status(len(bt.sizes)) == 0).all()
    return outs


def check_both(torch, c, bt, groups, outs, mean=None, std=None, reduce=0, what=""):
    assert isinstance(outs, list) and len(outs) == len(groups)
    for k, (g, out) in enumerate(zip(groups, outs)):
        assert out.dtype == g.get("dtype", torch.float32) and out.shape == (n_views(bt, g), 3, *g["size"]), (what, k, out.shape)
        assert_bits(torch, out, ref_numpy(torch, c, bt, g, mean, std, reduce), (what, "group", k, "ref_resize"))
        want = ref_resized(torch, c, bt, g, mean, std, reduce)
        assert torch.equal(out.view(torch.uint8), want.view(torch.uint8)), (what, "group", k, "decode_tensor_resized")


# ------------------------------------------------------------------------------------------------ 1. two groups in one call
@pytest.mark.parametrize("half", ["float16", "bfloat16"])
def test_two_groups_in_one_call(torch_mod, codec, half):
    torch = torch_mod
    bt = mixed(torch, codec)
    groups = [dict(G0, dtype=getattr(torch, half)), dict(G1, dtype=torch.float32)]
    outs = views(codec, bt, groups, mean=IMAGENET[0], std=IMAGENET[1])
    check_both(torch, codec, bt, groups, outs, *IMAGENET, what=half)


# ------------------------------------------------------------------------------------------------ 2. more views than one launch carries
def test_view_table_longer_than_one_slice(torch_mod, codec):
    """130 views of two images to (8, 12), the image index alternating: views 128 and 129 sit in the group's second launch and get THEIR image,
    box and flip."""
    torch = torch_mod
    from llicti_amd.codec import VIEW_SLICE
    assert VIEW_SLICE == 128
    bt = batch(torch, codec, SIZES[:2], seed=SEED)
    rng = np.random.default_rng(5)
    n = VIEW_SLICE + 2
    image = [v & 1 for v in range(n)]
    boxes = []
    for b in image:
        h, w = SIZES[b]
        hs, ws = int(rng.integers(1, min(h, 32) + 1)), int(rng.integers(1, min(w, 48) + 1))      # (at most 4 x the output: the filter takes it)
        boxes.append((int(rng.integers(0, h - hs + 1)), int(rng.integers(0, w - ws + 1)), hs, ws))
    g = dict(size=(8, 12), image=image, boxes=boxes, flip=[int(v) for v in rng.integers(0, 2, n)], antialias=True)
    (out,) = views(codec, bt, [g], mean=IMAGENET[0], std=IMAGENET[1])
    want = ref_numpy(torch, codec, bt, g, *IMAGENET)
    for v in (0, 1, VIEW_SLICE - 1, VIEW_SLICE, VIEW_SLICE + 1):
        assert_bits(torch, out[v], want[v], v)
    check_both(torch, codec, bt, [g], [out], *IMAGENET)


# ------------------------------------------------------------------------------------------------ 3. tile edges
def test_tile_edges(torch_mod, codec):
    """(17, 65): two 16 x 64 tiles on each axis, the second one row and one column wide; (16, 64): exactly one tile.  Both flags."""
    torch = torch_mod
    bt = mixed(torch, codec)
    image, boxes, flip = [2, 1, 0, 2], [(30, 0, 64, 67), (0, 0, 64, 96), (2, 3, 30, 41), (95, 66, 1, 1)], [0, 1, 1, 0]
    for aa in (True, False):
        groups = [dict(size=(17, 65), image=image, boxes=boxes, flip=flip, antialias=aa),
                  dict(size=(16, 64), image=image, boxes=boxes, flip=flip, antialias=aa, dtype=torch.float16)]
        check_both(torch, codec, bt, groups, views(codec, bt, groups), what=aa)


# ------------------------------------------------------------------------------------------------ 4. identity
def test_identity(torch_mod, codec):
    """image=None with n == B gives decode_tensor_resized's bytes (boxes given, and boxes None: the whole images); boxes of Ho x Wo give
    decode_tensor's bytes for the same origins."""
    torch = torch_mod
    c = codec
    bt = mixed(torch, c)
    boxes, flip = [(1, 2, 30, 40), (0, 0, 64, 96), (30, 5, 60, 61)], [0, 1, 1]
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        g = dict(size=(16, 24), image=None, boxes=boxes, flip=flip, dtype=dt)
        (out,) = views(c, bt, [g], mean=IMAGENET[0], std=IMAGENET[1])
        c.poison_workspace(POISON)
        want = c.decode_tensor_resized(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, (16, 24), boxes, dtype=dt, flip=flip, mean=IMAGENET[0], std=IMAGENET[1])
        c.check()
        assert torch.equal(out.view(torch.uint8), want.view(torch.uint8)), dt
        y0, x0 = [17, 0, 80], [23, 5, 43]
        g = dict(size=(16, 24), image=None, boxes=[(y, x, 16, 24) for y, x in zip(y0, x0)], flip=flip, dtype=dt)
        (out,) = views(c, bt, [g], mean=IMAGENET[0], std=IMAGENET[1])
        c.poison_workspace(POISON)
        want = c.decode_tensor(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, (16, 24), dtype=dt, origin=(y0, x0), flip=flip, mean=IMAGENET[0], std=IMAGENET[1])
        c.check()
        assert torch.equal(out.view(torch.uint8), want.view(torch.uint8)), ("decode_tensor", dt)
    g = dict(size=(16, 24), antialias=False)                    # (image None, boxes None: every whole image)
    check_both(torch, c, bt, [g], views(c, bt, [g]), what="defaults")


# ------------------------------------------------------------------------------------------------ 5. reduced
@pytest.mark.parametrize("reduce", [1, 2])
def test_views_of_a_reduced_decode(torch_mod, codec, reduce):
    """Boxes in the coordinates of the image decoded at reduce r; reference 1 resamples img[:, ::2^r, ::2^r]."""
    torch = torch_mod
    from llicti_amd.codec import reduced_dims
    bt = mixed(torch, codec)
    dims = [reduced_dims(h, w, reduce) for h, w in SIZES]
    image = [0, 1, 2, 2, 1, 0]
    size = (12, 12) if reduce == 1 else (6, 6)                  # (every box below shrinks by at most 4)
    boxes = [(0, 0, *dims[0]), (0, 0, *dims[1]), (0, 0, *dims[2]), (1, 2, dims[2][0] - 2, dims[2][1] - 3), (dims[1][0] - 1, dims[1][1] - 1, 1, 1), (1, 1, 5, 7)]
    assert all(h <= 4 * size[0] and w <= 4 * size[1] for _, _, h, w in boxes)
    groups = [dict(size=size, image=image, boxes=boxes, flip=[0, 1, 0, 1, 0, 1], dtype=torch.float16), dict(size=(5, 9), image=[2, 0], antialias=False)]
    outs = views(codec, bt, groups, mean=IMAGENET[0], std=IMAGENET[1], reduce=reduce)
    check_both(torch, codec, bt, groups, outs, *IMAGENET, reduce=reduce, what=reduce)


# ------------------------------------------------------------------------------------------------ 6. the reference format
def test_reference_format_two_views_per_image(torch_mod, codec):
    torch = torch_mod
    bt = batch(torch, codec, [(64, 96)] * 2, name="ac", seed=340)
    g = dict(size=(16, 24), image=[0, 0, 1, 1], boxes=[(0, 0, 64, 96), (7, 9, 40, 55), (3, 1, 20, 90), (60, 90, 4, 6)], flip=[1, 0, 0, 1], dtype=torch.bfloat16)
    check_both(torch, codec, bt, [g], views(codec, bt, [g], mean=IMAGENET[0], std=IMAGENET[1]), *IMAGENET, what="ac")


# ------------------------------------------------------------------------------------------------ 7. bounds
@pytest.mark.parametrize("size", [(16, 24), (15, 23)])
def test_nothing_outside_the_tensors(torch_mod, codec, size):
    """Every group's `out` is a view into a larger buffer of 0xA5, once at an offset that keeps 4-element stores (64 bytes) and once one element in
    (element stores): the bytes in front of and behind each tensor keep their value."""
    torch = torch_mod
    bt = mixed(torch, codec)
    specs = [dict(G0, size=size, dtype=torch.float32, antialias=False), dict(G1, size=size, dtype=torch.float16)]      # (64 rows to 15: not with the filter)
    for aligned in (True, False):
        bigs, groups = [], []
        for g in specs:
            es = torch.empty((), dtype=g["dtype"]).element_size()
            pad, nb = (64 if aligned else es), n_views(bt, g) * 3 * size[0] * size[1] * es
            big = torch.full((pad + nb + 64,), POISON, dtype=torch.uint8, device=DEV)
            bigs.append((big, pad, nb))
            groups.append(dict(g, out=big[pad:pad + nb].view(g["dtype"]).view(-1, 3, *size)))
        outs = views(codec, bt, groups)
        for g, out, (big, pad, nb) in zip(groups, outs, bigs):
            assert out.data_ptr() == big.data_ptr() + pad
            host = big.cpu()
            assert (host[:pad] == POISON).all() and (host[pad + nb:] == POISON).all(), (aligned, g["dtype"])
        check_both(torch, codec, bt, specs, outs, what=("aligned", aligned))


# ------------------------------------------------------------------------------------------------ 8. refusals
def _raw_call(torch, c, bt, arr, G):
    """the C call with a group table built by hand (what HipCodec.decode_tensor_views cannot express: null pointers, counts without arrays)"""
    from llicti_amd.codec import _ptr, _stream_ptr
    Hs, Ws = np.asarray(bt.Hs, dtype=np.int32), np.asarray(bt.Ws, dtype=np.int32)
    ws = c.workspace_v(Hs, Ws, bt.mode)
    modes = np.array([bt.mode], dtype=np.int32)
    rc = c.L.llicti_decode_images_tensor_views(c.ctx, _ptr(bt.cont), bt.cont.shape[1], _ptr(bt.seg), len(Hs), _ptr(Hs), _ptr(Ws), _ptr(modes), 1, 0,
                                               _ptr(ws), ws.numel(), arr, G, None, None, _stream_ptr(c.device))
    return rc, c.L.llicti_last_error().decode()


def test_refusals_are_einval_and_launch_nothing(torch_mod, codec):
    torch = torch_mod
    from llicti_amd import _lib
    from llicti_amd._lib import EINVAL, LlictiError
    c = codec
    bt = mixed(torch, c)
    views(c, bt, [G0, G1])
    o0 = torch.full((7, 3, 16, 24), float("nan"), device=DEV)
    o1 = torch.full((5, 3, 13, 19), float("nan"), device=DEV)
    good = [dict(G0, out=o0), dict(G1, out=o1)]

    def swap(g, v, box):
        return dict(good[g], boxes=[box if k == v else b for k, b in enumerate(good[g]["boxes"])])

    def names(g, v):
        return ("group %d" % g,) + (() if v is None else ("view %d" % v,))

    # (groups, keywords of the call) -> the words the message holds
    refused = [([good[0], swap(1, 3, (63, 0, 0, 96))], {}, names(1, 3)), ([swap(0, 2, (5, 7, 9, -11)), good[1]], {}, names(0, 2)),
               ([swap(0, 1, (0, 0, 34, 47)), good[1]], {}, names(0, 1) + ("image 0", "leaves")),            # one row too far: image 0 has 33
               ([good[0], swap(1, 2, (10, 95, 40, 2))], {}, names(1, 2) + ("leaves",)),                     # one column too far: 95 + 2 > 96
               ([swap(0, 6, (-1, 1, 31, 45)), good[1]], {}, names(0, 6)), ([swap(0, 6, (1, -1, 31, 45)), good[1]], {}, names(0, 6)),
               ([swap(0, 5, (31, 7, 65, 60)), good[1]], {}, names(0, 5) + ("raise reduce",)),               # 65 rows to 16 with the filter
               ([dict(size=(8, 8), image=[0], boxes=[(0, 0, 8, 8)], out=o0), swap(1, 0, (0, 0, 33, 48))], dict(reduce=1), names(1, 0)),      # image 1 at reduce 1 is 32 x 48
               ([dict(good[0], image=[2, 0, 0, 3, 2, 2, 0]), good[1]], {}, names(0, 3) + ("image 3",)),
               ([good[0], dict(good[1], image=[1, 1, 1, 1, -1])], {}, names(1, 4) + ("image -1",)),
               ([good[0], dict(good[1], antialias=2)], {}, names(1, None) + ("antialias",)), ([dict(good[0], antialias=-1)], {}, names(0, None) + ("antialias",)),
               ([good[0], dict(good[1], dtype=7)], {}, names(1, None) + ("dtype",)),
               ([good[0]], dict(mean=IMAGENET[0], std=(0.229, 0.0, 0.225)), ("std",)), ([good[0]], dict(mean=IMAGENET[0]), ("mean",)),
               ([good[0]], dict(std=IMAGENET[1]), ("mean",)), ([good[0]], dict(reduce=6), ("reduce",)), ([good[0]], dict(reduce=-1), ("reduce",)),
               ([], {}, ("0 groups",)), ([good[1]] * 17, {}, ("17 groups",))]
    before = {k: c.counter(k) for k in ("plan_builds", "plan_hits", "device_syncs", "device_allocs")}
    for groups, kw, words in refused:
        with pytest.raises(LlictiError) as e:
            c.decode_tensor_views(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, groups, **kw)
        assert e.value.code == EINVAL and all(w in str(e.value) for w in words), (words, str(e.value))
    for g, bad_size in [(0, (0, 24)), (1, (16, 0)), (0, (-3, 24)), (1, (8161, 2)), (0, (2, 8161))]:
        with pytest.raises(LlictiError) as e:
            c.decode_tensor_views(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, [dict(good[k], size=bad_size, antialias=False, out=None if max(bad_size) > 8160 else good[k]["out"]) if k == g else good[k]
                                                                                  for k in range(2)])
        assert e.value.code == EINVAL and "output size" in str(e.value) and "group %d" % g in str(e.value), (bad_size, str(e.value))
    # what only a hand-built table holds: null groups, a null d_out, n outside 1 .. 2^20, image NULL with n != B
    rc, msg = _raw_call(torch, c, bt, None, 1)
    assert rc == EINVAL and "null groups" in msg
    arr = (_lib.ViewGroup * 2)()
    o2 = torch.full((3, 3, 16, 24), float("nan"), device=DEV)
    for vg, o, (Ho, Wo) in zip(arr, (o2, o1), ((16, 24), (13, 19))):
        vg.d_out, vg.dtype, vg.Ho, vg.Wo, vg.antialias, vg.n = o.data_ptr(), 0, Ho, Wo, 0, 3
    for field, value, words in (("d_out", None, ("group 1", "d_out")), ("n", 0, ("group 1", "n = 0")), ("n", -4, ("group 1", "n = -4")),
                                ("n", (1 << 20) + 1, ("group 1", "n = 1048577")), ("n", 2, ("group 1", "n = 2", "3 images")), ("n", 4, ("group 1", "n = 4"))):
        keep = getattr(arr[1], field)
        setattr(arr[1], field, value)
        rc, msg = _raw_call(torch, c, bt, arr, 2)
        assert rc == EINVAL and all(w in msg for w in words), (field, value, msg)
        setattr(arr[1], field, keep)
    assert {k: c.counter(k) for k in before} == before
    assert torch.isnan(o0).all() and torch.isnan(o1).all() and torch.isnan(o2).all()                         # nothing was written ...
    c.check()                                                                      # ... launched or latched
    # the filter's limit does not bind without the filter; the hand-built table, untouched, is a valid call (two identity groups)
    (got,) = views(c, bt, [dict(swap(0, 5, (31, 7, 65, 60)), antialias=False, out=None)])
    assert got.shape == (7, 3, 16, 24)
    rc, msg = _raw_call(torch, c, bt, arr, 2)
    assert rc == 0, msg
    c.check()
    assert not torch.isnan(o2).any() and not torch.isnan(o1[:3]).any()
    assert {k: c.counter(k) for k in before} == {**before, "plan_hits": before["plan_hits"] + 2}      # (the two valid calls)


# ------------------------------------------------------------------------------------------------ 9. no host cost
def test_fresh_views_every_call_cost_plan_hits_only(torch_mod, codec):
    torch = torch_mod
    c = codec
    bt = mixed(torch, c)
    c.poison_workspace(POISON)
    c.decode_reduced(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, 0)                      # the plan of (sizes, mode, reduce 0) -- decode_reduced's
    c.check()
    before = {k: c.counter(k) for k in ("plan_builds", "plan_hits", "device_syncs", "device_allocs")}
    rng = np.random.default_rng(13)
    calls = []
    for _ in range(4):
        groups = []
        for _g in range(2):
            size = (int(rng.integers(8, 30)), int(rng.integers(8, 30)))
            n = int(rng.integers(1, 9))
            image = [int(v) for v in rng.integers(0, 3, n)]
            boxes = []
            for b in image:
                h, w = SIZES[b]
                hs, ws = int(rng.integers(1, min(h, 4 * size[0]) + 1)), int(rng.integers(1, min(w, 4 * size[1]) + 1))
                boxes.append((int(rng.integers(0, h - hs + 1)), int(rng.integers(0, w - ws + 1)), hs, ws))
            groups.append(dict(size=size, image=image, boxes=boxes, flip=[int(v) for v in rng.integers(0, 2, n)], antialias=bool(rng.integers(0, 2))))
        calls.append((groups, c.decode_tensor_views(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, groups, mean=IMAGENET[0], std=IMAGENET[1])))
    after = {k: c.counter(k) for k in before}
    assert after == {**before, "plan_hits": before["plan_hits"] + 4}, (before, after)    # the first views call hit decode_reduced's plan
    c.check()
    for groups, outs in calls:
        for g, out in zip(groups, outs):
            assert_bits(torch, out, ref_numpy(torch, c, bt, g, *IMAGENET), g)


# ------------------------------------------------------------------------------------------------ 10. status
def test_a_damaged_container_no_view_names(torch_mod, codec):
    """Image 1's container gets the retired v2 tag in header byte 0 (a reported error, never a fault) and NO view names image 1: its status word
    alone is set all the same, and the views of images 0 and 2 are exact."""
    torch = torch_mod
    from llicti_amd._lib import EFORMAT, LlictiError
    c = codec
    bt = mixed(torch, c)
    bad = bt.cont.clone()
    bad[1, 0] = 0x95
    g = dict(size=(16, 24), image=[2, 0, 0, 2], boxes=[G0["boxes"][k] for k in (0, 1, 2, 5)], flip=[1, 0, 1, 0], dtype=torch.float16)
    c.poison_workspace(POISON)
    (out,) = c.decode_tensor_views(bad, bt.seg, bt.Hs, bt.Ws, bt.mode, [g], mean=IMAGENET[0], std=IMAGENET[1])
    with pytest.raises(LlictiError) as e:
        c.check()
    assert e.value.code == EFORMAT
    assert list(c.image_status(3)) == [0, EFORMAT, 0]
    c.check()                                          # (read and cleared)
    assert_bits(torch, out, ref_numpy(torch, c, bt, g, *IMAGENET), "views of the good images")
    want = ref_resized(torch, c, bt, g, *IMAGENET)
    assert torch.equal(out.view(torch.uint8), want.view(torch.uint8))
    # the resized call on the same containers reports the same words
    c.decode_tensor_resized(bad, bt.seg, bt.Hs, bt.Ws, bt.mode, (16, 24), None, antialias=False)
    assert list(c.image_status(3)) == [0, EFORMAT, 0]
    with pytest.raises(LlictiError):
        c.check()
    c.check()


# ------------------------------------------------------------------------------------------------ 11. ordering
def test_on_a_callers_stream_behind_a_gate(torch_mod, codec):
    """The call on a caller's non-blocking stream that a gate (helpers.StreamGate) holds busy: the containers it reads are DECOYS until a copy,
    enqueued on that stream behind the gate, overwrites them; both groups' results are copied out on the stream.  Everything is enqueued before
    the gate ends (asserted), so a launch that was not ordered on the stream would have decoded the decoys."""
    torch = torch_mod
    c = codec
    bt = mixed(torch, c)
    decoy = batch(torch, c, SIZES, seed=900)
    assert bt.cont.shape == decoy.cont.shape and not torch.equal(bt.cont, decoy.cont)
    groups = [dict(G0, dtype=torch.float16), G1]
    want = [ref_numpy(torch, c, bt, g, *IMAGENET) for g in groups]
    s = torch.cuda.Stream(device=DEV)
    gate = StreamGate(torch, DEV)
    with torch.cuda.stream(s):                          # warm on this stream: kernels loaded, plan cached, workspace there
        views(c, bt, groups, mean=IMAGENET[0], std=IMAGENET[1])
    torch.cuda.synchronize()
    cont, seg = decoy.cont.clone(), decoy.seg.clone()
    outs = [torch.full((7, 3, 16, 24), float("nan"), dtype=torch.float16, device=DEV), torch.full((5, 3, 13, 19), float("nan"), device=DEV)]
    c.poison_workspace(POISON)
    torch.cuda.synchronize()
    begin, end = gate.hold(s, 100.0)
    with torch.cuda.stream(s):
        cont.copy_(bt.cont, non_blocking=True)
        seg.copy_(bt.seg, non_blocking=True)
        c.decode_tensor_views(cont, seg, bt.Hs, bt.Ws, bt.mode, [dict(g, out=o) for g, o in zip(groups, outs)], mean=IMAGENET[0], std=IMAGENET[1])
        got = [torch.empty_like(o) for o in outs]
        for a, o in zip(got, outs):
            a.copy_(o, non_blocking=True)
    assert not end.query(), "the gate ended before the last enqueue: the run proves nothing"
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c.check()
    for k in range(2):
        assert_bits(torch, got[k], want[k], ("gated", k))


# ------------------------------------------------------------------------------------------------ 12. the model layer
def test_model_layer_dispatches_views(torch_mod):
    """LLICTI.decode_batch_async(tensor=dict(views=...)) on a list of mixed sizes, with multi_crop_plan's reduce and boxes: the list of tensors."""
    torch = torch_mod
    from helpers import make_image
    from llicti_amd.codec import multi_crop_plan
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    torch.manual_seed(1337)
    m = LLICTI(default_config(container="xrans2")).to(DEV).eval()
    dev = torch.device(DEV)
    sizes = [(150, 131), (96, 160)]
    rgbs = [make_image("smooth", h, w, 40 + i) for i, (h, w) in enumerate(sizes)]
    lists = m.encode_batch_async(rgbs).lists()
    full = [((32, 28), [0, 1, 1], [(3, 8, 140, 120), (0, 20, 96, 130), (10, 0, 80, 70)]), ((12, 12), [1, 0], [(40, 50, 30, 30), (100, 90, 50, 41)])]
    reduce, boxes = multi_crop_plan(sizes, full)
    assert reduce == 1 and boxes[0][0] == (2, 4, 70, 60) and boxes[1][0] == (20, 25, 15, 15)       # (the 30 x 30 box keeps 15 >= 12 pixels at r = 1, 8 at r = 2)
    groups = [dict(size=(32, 28), image=[0, 1, 1], boxes=boxes[0], flip=[1, 0, 1], dtype=torch.float16), dict(size=(12, 12), image=[1, 0], boxes=boxes[1])]
    m.codec().poison_workspace()
    got = m.decode_batch_async(lists, dev, reduce=reduce, tensor=dict(views=groups, mean=IMAGENET[0], std=IMAGENET[1]))
    m.codec().check()
    assert isinstance(got, list) and len(got) == 2
    for g, out in zip(groups, got):
        want = np.stack([rr.resized_crop(rgbs[b][:, ::2, ::2], box, g["size"], 1, bool(f), *IMAGENET, tname(torch, g.get("dtype", torch.float32)))
                         for b, box, f in zip(g["image"], g["boxes"], g.get("flip") or [0] * len(g["image"]))])
        assert_bits(torch, out, want, g["size"])
    for extra in (dict(size=(8, 8)), dict(boxes=boxes[0]), dict(origin=([0, 0], [0, 0]))):
        with pytest.raises(ValueError):
            m.decode_batch_async(lists, dev, reduce=reduce, tensor=dict(views=groups, **extra))
