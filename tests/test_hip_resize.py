"""Resized crops on the GPU (run with -m gpu on an MI355X): llicti_decode_images_tensor_resized resamples a source box per image to one dense
[B, 3, Ho, Wo] tensor in the decode's last kernel.  Every check is EXACT (bit for bit).  The reference is always the ORIGINAL pixels -- the
images the containers were made from -- through tests/ref_resize.py, the numpy float32 restatement of the arithmetic in include/llicti_hip.h;
never the code under test.  Images: helpers.make_image at 67x93, 64x96, 96x64 and 33x32, "trainedlike" weights, xrans2 containers (the reference
format for one equal-size case); every decode runs on a poisoned workspace."""
import numpy as np
import pytest

import ref_resize as rr
from conftest import load_state_dict
from helpers import StreamGate, make_image

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [(67, 93), (64, 96), (96, 64), (33, 32)]
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
POISON = 0xA5
OUT = (16, 24)
# the boxes of test 1, (y0, x0, hs, ws) per image of SIZES: the whole image, an odd interior box, a 1 x 1 box, a box ending at the bottom-right pixel
WHOLE = [(0, 0, h, w) for h, w in SIZES]
INTERIOR = [(3, 5, 61, 77), (1, 7, 51, 83), (5, 3, 63, 55), (3, 5, 27, 21)]
ONE = [(h // 2, w // 3, 1, 1) for h, w in SIZES]
CORNER = [(h - 29, w - 31, 29, 31) for h, w in SIZES]
FLIP = [0, 0, 1, 0]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def codec(torch_mod):
    from llicti_amd.codec import HipCodec
    c = HipCodec(DEV)
    c.load_state_dict(load_state_dict("trainedlike"))
    yield c
    c.set_profiling(False)
    c.close()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Batch:
    """One encoded batch, made once: the original images on the host (the reference's input) and their containers on the device."""

    def __init__(self, torch, c, sizes, name="xrans2", seed=300):
        from llicti_amd.codec import mode_of_name
        self.sizes = list(sizes)
        self.Hs, self.Ws = [h for h, _ in sizes], [w for _, w in sizes]
        self.rgbs = [make_image(("smooth", "noise")[i % 2], h, w, seed + i) for i, (h, w) in enumerate(sizes)]
        self.mode = mode_of_name(name)
        if len(set(self.sizes)) == 1:
            self.cont, self.seg = c.encode(_dev(torch, np.stack(self.rgbs)), mode=self.mode)
        else:
            self.cont, self.seg = c.encode_v(_dev(torch, np.concatenate([r.reshape(-1) for r in self.rgbs])), self.Hs, self.Ws, self.mode)
        c.check()
        c.workspace_v(self.Hs, self.Ws, self.mode)


_BATCHES, _RESAMPLED = {}, {}


def batch(torch, c, sizes=SIZES, name="xrans2", seed=300):
    key = (tuple(sizes), name, seed)
    if key not in _BATCHES:
        _BATCHES[key] = Batch(torch, c, sizes, name, seed)
    return _BATCHES[key]


def reference(bt, boxes, size, antialias, flip=None, mean=None, std=None, dtype="float32", reduce=0, key=None):
    """[B, 3, Ho, Wo] float32 values of the output tensor: the original pixels (decimated by 2^reduce) through ref_resize.  The resampled planes
    (before / 255, normalise and dtype) are computed once per (batch, boxes, size, flag, reduce) and shared."""
    out = []
    for b, rgb in enumerate(bt.rgbs):
        k = (key or id(bt), b, tuple(boxes[b]), tuple(size), int(antialias), reduce)
        if k not in _RESAMPLED:
            y0, x0, hs, ws = boxes[b]
            src = rgb[:, ::1 << reduce, ::1 << reduce][:, y0:y0 + hs, x0:x0 + ws]
            assert src.shape == (3, hs, ws)
            _RESAMPLED[k] = rr.resample(src, size[0], size[1], antialias)
        v = rr.finish(_RESAMPLED[k], mean, std, dtype)
        out.append(v[:, :, ::-1] if flip is not None and flip[b] else v)
    return np.stack(out)


def tname(torch, dt):
    return {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}[dt]


def bits(torch, t):
    """a tensor's values as float32 bit patterns on the host (every float16 / bfloat16 value is a float32 value)"""
    return t.detach().float().cpu().contiguous().numpy().view(np.uint32)


def assert_bits(torch, got, want, what):
    g, w = bits(torch, got), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError((what, "%d of %d values differ; first at %s: got %r, want %r" % (len(bad), g.size, i, g.view(np.float32)[i], w.view(np.float32)[i])))


def resized(c, bt, size, boxes, **kw):
    c.poison_workspace(POISON)
    out = c.decode_tensor_resized(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size, boxes, **kw)
    c.check()
    assert (c.image_status(len(bt.sizes)) == 0).all()
    return out


# ------------------------------------------------------------------------------------------------ 1. the mixed batch
@pytest.mark.parametrize("norm", [None, IMAGENET], ids=["plain", "imagenet"])
@pytest.mark.parametrize("dt", ["float32", "float16", "bfloat16"])
def test_mixed_batch_to_16x24(torch_mod, codec, dt, norm):
    """Four images of four sizes into one [4, 3, 16, 24] tensor, image 2 mirrored, both filter flags, four box sets.  The whole images of 67 and 96
    rows shrink to 16 rows by more than 4: with the filter on, that box set is REFUSED at reduce 0 (the header's rule; asserted here) and run at
    reduce 1 instead -- what the refusal tells a caller to do; without the filter it runs at reduce 0."""
    torch = torch_mod
    from llicti_amd._lib import EINVAL, LlictiError
    c = codec
    bt = batch(torch, c)
    tdt = getattr(torch, dt)
    mean, std = norm if norm else (None, None)
    for aa in (0, 1):
        for name, boxes in (("whole", WHOLE), ("interior", INTERIOR), ("one", ONE), ("corner", CORNER)):
            if name == "whole" and aa:
                with pytest.raises(LlictiError) as e:
                    c.decode_tensor_resized(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, OUT, boxes, antialias=True)
                assert e.value.code == EINVAL and "image 0" in str(e.value) and "raise reduce" in str(e.value)
                red = [(0, 0, -(-h // 2), -(-w // 2)) for h, w in SIZES]
                got = resized(c, bt, OUT, red, dtype=tdt, flip=FLIP, mean=mean, std=std, antialias=True, reduce=1)
                assert_bits(torch, got, reference(bt, red, OUT, 1, FLIP, mean, std, dt, reduce=1), (name, "reduce 1"))
                continue
            got = resized(c, bt, OUT, boxes, dtype=tdt, flip=FLIP, mean=mean, std=std, antialias=bool(aa))
            assert got.dtype == tdt and got.shape == (4, 3, *OUT)
            assert_bits(torch, got, reference(bt, boxes, OUT, aa, FLIP, mean, std, dt), (name, aa))
    # boxes = None: every whole image (the NULL defaults of the C call)
    got = resized(c, bt, OUT, None, dtype=tdt, mean=mean, std=std, antialias=False)
    assert_bits(torch, got, reference(bt, WHOLE, OUT, 0, None, mean, std, dt), "boxes None")


# ------------------------------------------------------------------------------------------------ 2. scales, store paths
SCALES = [("exactly 4", 1, (0, 0, 64, 96), (16, 24)), ("2.3 down", 0, (0, 0, 67, 93), (29, 40)), ("1.7 up", 3, (0, 0, 33, 32), (56, 54)),
          ("tall to wide", 2, (2, 10, 60, 20), (16, 48)), ("Wo = 23", 1, (0, 2, 64, 92), (16, 23))]


@pytest.mark.parametrize("what,img,box,size", SCALES, ids=[s[0] for s in SCALES])
def test_scales(torch_mod, codec, what, img, box, size):
    """One image per call, both flags and a mirrored run: a scale of exactly 4.0 with the filter (8 taps), 2.3 x down, 1.7 x up, a tall box to a
    wide output, and an odd output width (element-by-element stores)."""
    torch = torch_mod
    c = codec
    bt = batch(torch, c, [SIZES[img]], seed=300 + img)
    for aa in (1, 0):
        for flip in ([0], [1]):
            got = resized(c, bt, size, [box], flip=flip, antialias=bool(aa), mean=IMAGENET[0], std=IMAGENET[1])
            assert_bits(torch, got, reference(bt, [box], size, aa, flip, *IMAGENET), (what, aa, flip))


def test_unaligned_then_aligned_out(torch_mod, codec):
    """The same call into an `out` view whose base is one element past a 4-element boundary (scalar stores) and into an aligned one (4-element
    stores): the same values, float32 and float16."""
    torch = torch_mod
    c = codec
    bt = batch(torch, c)
    n = 4 * 3 * OUT[0] * OUT[1]
    for dt in (torch.float32, torch.float16):
        want = reference(bt, INTERIOR, OUT, 1, FLIP, *IMAGENET, tname(torch, dt))
        for shift in (1, 4, 0):
            big = torch.zeros(n + 8, dtype=dt, device=DEV)
            out = big[shift:shift + n].view(4, 3, *OUT)
            got = resized(c, bt, OUT, INTERIOR, dtype=dt, flip=FLIP, mean=IMAGENET[0], std=IMAGENET[1], out=out)
            assert got.data_ptr() == big.data_ptr() + shift * big.element_size()
            assert_bits(torch, got, want, (dt, shift))


def test_reference_format_equal_sizes(torch_mod, codec):
    torch = torch_mod
    c = codec
    bt = batch(torch, c, [(64, 96)] * 2, name="ac", seed=340)
    boxes = [(0, 0, 64, 96), (7, 9, 40, 55)]
    got = resized(c, bt, OUT, boxes, dtype=torch.bfloat16, flip=[1, 0], mean=IMAGENET[0], std=IMAGENET[1])
    assert_bits(torch, got, reference(bt, boxes, OUT, 1, [1, 0], *IMAGENET, "bfloat16"), "ac")


# ------------------------------------------------------------------------------------------------ 3. identity
def test_identity_is_decode_tensor(torch_mod, codec):
    """A box of Ho x Wo (scale 1) gives the BYTES of decode_tensor for the same origin, flip, normalisation and dtype -- at reduce 0 and 1."""
    torch = torch_mod
    c = codec
    bt = batch(torch, c)
    for reduce, size, y0, x0 in ((0, (16, 24), [51, 0, 33, 17], [69, 5, 0, 8]), (1, (16, 16), [18, 0, 7, 1], [31, 3, 16, 0])):
        boxes = [(y, x, size[0], size[1]) for y, x in zip(y0, x0)]
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            for aa in (True, False):
                c.poison_workspace(POISON)
                want = c.decode_tensor(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size, dtype=dt, origin=(y0, x0), flip=FLIP, mean=IMAGENET[0], std=IMAGENET[1], reduce=reduce)
                c.check()
                got = resized(c, bt, size, boxes, dtype=dt, flip=FLIP, mean=IMAGENET[0], std=IMAGENET[1], antialias=aa, reduce=reduce)
                assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), (reduce, dt, aa)
        got = resized(c, bt, size, boxes, reduce=reduce)          # (and against the original pixels)
        assert_bits(torch, got, reference(bt, boxes, size, 1, reduce=reduce), ("pixels", reduce))


# ------------------------------------------------------------------------------------------------ 4. reduced
@pytest.mark.parametrize("reduce", [1, 2])
def test_boxes_of_a_reduced_decode(torch_mod, codec, reduce):
    """Boxes in the coordinates of the image decoded at reduce r; the reference resamples img[:, ::2^r, ::2^r].  Under profiling the call reports no
    more band-CNN launches than decode_reduced at that r: the finer levels are never decoded."""
    torch = torch_mod
    from llicti_amd.codec import reduced_dims
    c = codec
    bt = batch(torch, c)
    dims = [reduced_dims(h, w, reduce) for h, w in SIZES]
    size = (12, 12) if reduce == 1 else (7, 8)             # (every box below shrinks by at most 4: both flags run on all of them)
    sets = [[(0, 0, h, w) for h, w in dims], [(1, 2, h - 2, w - 3) for h, w in dims], [(h - 1, w - 1, 1, 1) for h, w in dims]]
    c.set_profiling(True)
    try:
        c.poison_workspace(POISON)
        c.decode_reduced(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, reduce)
        c.check()
        n_reduced = c.last_timing()[1]
        assert n_reduced == 3 * (5 - reduce)
        for boxes in sets:
            for aa in (1, 0):
                assert all(h <= 4 * size[0] and w <= 4 * size[1] for _, _, h, w in boxes)
                got = resized(c, bt, size, boxes, flip=FLIP, antialias=bool(aa), reduce=reduce, dtype=torch.float16, mean=IMAGENET[0], std=IMAGENET[1])
                assert c.last_timing()[1] <= n_reduced, (reduce, c.last_timing()[1], n_reduced)
                assert_bits(torch, got, reference(bt, boxes, size, aa, FLIP, *IMAGENET, "float16", reduce=reduce), (reduce, boxes[0], aa))
    finally:
        c.set_profiling(False)


# ------------------------------------------------------------------------------------------------ 5. more boxes than one launch carries
def test_box_table_longer_than_one_slice(torch_mod, codec):
    """B = slice + 2 images of 32 x 32 in one call (two launches of the last kernel): the first, the two around the boundary and the last image
    each get THEIR box, flip and status word."""
    torch = torch_mod
    from llicti_amd.codec import RESIZE_BOX_SLICE
    c = codec
    B = RESIZE_BOX_SLICE + 2
    bt = batch(torch, c, [(32, 32)] * B, seed=500)
    rng = np.random.default_rng(77)
    boxes = []
    for b in range(B):
        hs, ws = int(rng.integers(1, 33)), int(rng.integers(1, 33))
        boxes.append((int(rng.integers(0, 33 - hs)), int(rng.integers(0, 33 - ws)), hs, ws))
    flip = [int(v) for v in rng.integers(0, 2, B)]
    size = (9, 12)
    got = resized(c, bt, size, boxes, flip=flip, antialias=True, mean=IMAGENET[0], std=IMAGENET[1])
    assert got.shape == (B, 3, 9, 12)
    assert (c.image_status(B) == 0).all()
    want = reference(bt, boxes, size, 1, flip, *IMAGENET)
    for b in (0, 1, RESIZE_BOX_SLICE - 1, RESIZE_BOX_SLICE, RESIZE_BOX_SLICE + 1):
        assert_bits(torch, got[b], want[b], b)
    assert_bits(torch, got, want, "all")


# ------------------------------------------------------------------------------------------------ 6. bounds
@pytest.mark.parametrize("size", [(16, 24), (15, 23)])
def test_nothing_outside_the_tensor(torch_mod, codec, size):
    """`out` is a view into a larger buffer of 0xA5, at an offset that keeps 4-element stores (64 bytes) and at one that forbids them (one
    element): the bytes in front of and behind the tensor keep their value."""
    torch = torch_mod
    c = codec
    bt = batch(torch, c)
    n = 4 * 3 * size[0] * size[1]
    for dt in (torch.float32, torch.float16):
        es = torch.empty((), dtype=dt).element_size()
        want = reference(bt, CORNER, size, 1, FLIP, dtype=tname(torch, dt))
        for pad in (64, es):
            big = torch.full((pad + n * es + 64,), POISON, dtype=torch.uint8, device=DEV)
            out = big[pad:pad + n * es].view(dt).view(4, 3, *size)
            got = resized(c, bt, size, CORNER, dtype=dt, flip=FLIP, out=out)
            assert got.data_ptr() == big.data_ptr() + pad
            host = big.cpu()
            assert (host[:pad] == POISON).all() and (host[pad + n * es:] == POISON).all(), (dt, pad)
            assert_bits(torch, host[pad:pad + n * es].view(dt).view(4, 3, *size), want, (dt, pad))


# ------------------------------------------------------------------------------------------------ 7. no host cost
def test_fresh_boxes_every_call_cost_nothing_on_the_host(torch_mod, codec):
    torch = torch_mod
    c = codec
    bt = batch(torch, c)
    resized(c, bt, OUT, INTERIOR)                                              # warm: the plan of (sizes, mode, reduce 0)
    before = {k: c.counter(k) for k in ("plan_builds", "plan_hits", "device_syncs", "device_allocs")}
    rng = np.random.default_rng(11)
    calls = []
    for _ in range(20):
        size = (int(rng.integers(8, 40)), int(rng.integers(8, 40)))
        boxes = []
        for h, w in SIZES:
            hs, ws = int(rng.integers(1, min(h, 4 * size[0]) + 1)), int(rng.integers(1, min(w, 4 * size[1]) + 1))
            boxes.append((int(rng.integers(0, h - hs + 1)), int(rng.integers(0, w - ws + 1)), hs, ws))
        flip = [int(v) for v in rng.integers(0, 2, 4)]
        aa = int(rng.integers(0, 2))
        out = c.decode_tensor_resized(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, size, boxes, flip=flip, antialias=bool(aa), mean=IMAGENET[0], std=IMAGENET[1])
        calls.append((size, boxes, flip, aa, out))
    after = {k: c.counter(k) for k in before}
    assert after["plan_builds"] == before["plan_builds"] and after["plan_hits"] == before["plan_hits"] + 20, (before, after)
    assert after["device_syncs"] == before["device_syncs"] and after["device_allocs"] == before["device_allocs"], (before, after)
    c.check()
    for size, boxes, flip, aa, out in calls:
        assert_bits(torch, out, reference(bt, boxes, size, aa, flip, *IMAGENET), (size, boxes, flip, aa))
    # ... and that plan is llicti_decode_images_reduced's: the planar call on the same batch finds it
    c.decode_reduced(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, 0)
    c.check()
    assert c.counter("plan_builds") == after["plan_builds"] and c.counter("plan_hits") == after["plan_hits"] + 1


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_are_einval_and_launch_nothing(torch_mod, codec):
    torch = torch_mod
    from llicti_amd._lib import EINVAL, LlictiError
    c = codec
    bt = batch(torch, c)
    resized(c, bt, OUT, INTERIOR)
    c.check()

    def swap(b, box):
        return [box if k == b else v for k, v in enumerate(INTERIOR)]

    refused = [(dict(boxes=swap(1, (1, 7, 0, 83))), "image 1"), (dict(boxes=swap(2, (5, 3, 63, 0))), "image 2"), (dict(boxes=swap(3, (3, 5, -2, 21))), "image 3"),
               (dict(boxes=swap(1, (1, 7, 64, 83))), "image 1"),              # one row too far: 1 + 64 > 64
               (dict(boxes=swap(0, (3, 5, 61, 89))), "image 0"),              # one column too far: 5 + 89 > 93
               (dict(boxes=swap(2, (-1, 3, 63, 55))), "image 2"), (dict(boxes=swap(2, (5, -1, 63, 55))), "image 2"),
               (dict(boxes=[(0, 0, 8, 8)] * 3 + [(0, 0, 17, 17)], reduce=1), "image 3"),      # 33 x 32 at reduce 1 is 17 x 16
               (dict(antialias=2), "antialias"), (dict(antialias=-1), "antialias"),
               (dict(boxes=swap(0, (0, 0, 65, 77))), "raise reduce"),         # 65 rows to 16 with the filter: above 4 (64 are taken: test_scales)
               (dict(boxes=swap(2, (0, 0, 63, 61)), size=(16, 15)), "raise reduce"),
               (dict(mean=IMAGENET[0], std=(0.229, 0.0, 0.225)), "std"), (dict(mean=IMAGENET[0]), "mean"), (dict(std=IMAGENET[1]), "mean"),
               (dict(dtype=7), "dtype"), (dict(reduce=6), "reduce"), (dict(reduce=-1), "reduce")]
    before = {k: c.counter(k) for k in ("plan_builds", "plan_hits", "device_syncs", "device_allocs")}
    out = torch.full((4, 3, *OUT), float("nan"), device=DEV)
    for kw, word in refused:
        kw = dict(kw)
        with pytest.raises(LlictiError) as e:
            c.decode_tensor_resized(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, kw.pop("size", OUT), kw.pop("boxes", INTERIOR), out=out, **kw)
        assert e.value.code == EINVAL and word in str(e.value), (kw, str(e.value))
    for bad_size in ((0, 24), (16, 0), (-3, 24), (8161, 2), (2, 8161)):
        big = None if max(bad_size) > 8160 else out
        with pytest.raises(LlictiError) as e:
            c.decode_tensor_resized(bt.cont, bt.seg, bt.Hs, bt.Ws, bt.mode, bad_size, INTERIOR, antialias=False, out=big)
        assert e.value.code == EINVAL and "output size" in str(e.value), (bad_size, str(e.value))
    # the filter's limit does not bind without the filter
    got = resized(c, bt, OUT, [(0, 0, 65, 77), INTERIOR[1], INTERIOR[2], INTERIOR[3]], antialias=False)
    assert got.shape == (4, 3, *OUT)
    assert {k: c.counter(k) for k in before} == {**before, "plan_hits": before["plan_hits"] + 1}      # (the one valid call)
    assert torch.isnan(out).all()                                              # nothing was written ...
    c.check()                                                                  # ... launched or latched


# ------------------------------------------------------------------------------------------------ 9. status
def test_one_bad_container_among_good_ones(torch_mod, codec):
    """Image 1's container gets the retired v2 tag in header byte 0 (a reported error, never a fault): its status word alone is set, the other
    images' tensors are exact, and the bytes around `out` keep their value."""
    torch = torch_mod
    from llicti_amd._lib import EFORMAT, LlictiError
    c = codec
    bt = batch(torch, c)
    bad = bt.cont.clone()
    bad[1, 0] = 0x95
    n, pad = 4 * 3 * OUT[0] * OUT[1] * 4, 64
    big = torch.full((pad + n + 64,), POISON, dtype=torch.uint8, device=DEV)
    out = big[pad:pad + n].view(torch.float32).view(4, 3, *OUT)
    c.poison_workspace(POISON)
    c.decode_tensor_resized(bad, bt.seg, bt.Hs, bt.Ws, bt.mode, OUT, INTERIOR, flip=FLIP, mean=IMAGENET[0], std=IMAGENET[1], out=out)
    with pytest.raises(LlictiError) as e:
        c.check()
    assert e.value.code == EFORMAT
    assert list(c.image_status(4)) == [0, EFORMAT, 0, 0]
    c.check()                                          # (read and cleared)
    want = reference(bt, INTERIOR, OUT, 1, FLIP, *IMAGENET)
    host = big.cpu()
    assert (host[:pad] == POISON).all() and (host[pad + n:] == POISON).all()
    for b in (0, 2, 3):
        assert_bits(torch, out[b], want[b], b)
    assert_bits(torch, resized(c, bt, OUT, INTERIOR, flip=FLIP, mean=IMAGENET[0], std=IMAGENET[1]), want, "valid batch")


# ------------------------------------------------------------------------------------------------ 10. ordering
def test_on_a_callers_stream_behind_a_gate(torch_mod, codec):
    """The call on a caller's non-blocking stream that a gate (helpers.StreamGate) holds busy: the containers the call reads are DECOYS until a
    copy, enqueued on that stream behind the gate, overwrites them; the result is copied out on the stream.  Everything is enqueued before the
    gate ends (asserted), so a launch that was not ordered on the stream would have decoded the decoys."""
    torch = torch_mod
    c = codec
    bt = batch(torch, c)
    decoy = batch(torch, c, seed=900)
    assert bt.cont.shape == decoy.cont.shape and not torch.equal(bt.cont, decoy.cont)
    s = torch.cuda.Stream(device=DEV)
    gate = StreamGate(torch, DEV)
    kw = dict(dtype=torch.float16, flip=FLIP, mean=IMAGENET[0], std=IMAGENET[1])
    with torch.cuda.stream(s):                          # warm on this stream: kernels loaded, plan cached, workspace there
        resized(c, bt, OUT, INTERIOR, **kw)
    torch.cuda.synchronize()
    cont, seg = decoy.cont.clone(), decoy.seg.clone()
    out = torch.full((4, 3, *OUT), float("nan"), dtype=torch.float16, device=DEV)
    c.poison_workspace(POISON)
    torch.cuda.synchronize()
    begin, end = gate.hold(s, 100.0)
    with torch.cuda.stream(s):
        cont.copy_(bt.cont, non_blocking=True)
        seg.copy_(bt.seg, non_blocking=True)
        c.decode_tensor_resized(cont, seg, bt.Hs, bt.Ws, bt.mode, OUT, INTERIOR, out=out, **kw)
        got = torch.empty_like(out)
        got.copy_(out, non_blocking=True)
    assert not end.query(), "the gate ended before the last enqueue: the run proves nothing"
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c.check()
    assert_bits(torch, got, reference(bt, INTERIOR, OUT, 1, FLIP, *IMAGENET, "float16"), "gated")


# ------------------------------------------------------------------------------------------------ the model layer
def test_model_layer_dispatches_boxes(torch_mod):
    """LLICTI.decode_batch_async(tensor=dict(boxes=...)) on a list of mixed sizes: resized_crop_plan's reduce and boxes, one dense tensor; without
    `boxes` the same dict is a plain window, as before."""
    torch = torch_mod
    from llicti_amd.codec import resized_crop_plan
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    torch.manual_seed(1337)
    m = LLICTI(default_config(container="xrans2")).to(DEV).eval()
    dev = torch.device(DEV)
    sizes = [(150, 131), (96, 160)]
    rgbs = [make_image("smooth", h, w, 40 + i) for i, (h, w) in enumerate(sizes)]
    lists = m.encode_batch_async(rgbs).lists()
    full = [(3, 8, 140, 120), (0, 20, 96, 130)]
    size = (32, 28)
    reduce, boxes = resized_crop_plan(sizes, full, size)
    assert (reduce, boxes) == (1, [(2, 4, 70, 60), (0, 10, 48, 65)])          # (at r = 2 image 1's box would keep 24 rows: fewer than 32)
    m.codec().poison_workspace()
    got = m.decode_batch_async(lists, dev, reduce=reduce, tensor=dict(size=size, boxes=boxes, antialias=True, dtype=torch.float16, flip=[1, 0],
                                                                      mean=IMAGENET[0], std=IMAGENET[1]))
    m.codec().check()

    class _B:
        pass
    bt = _B()
    bt.rgbs = rgbs
    assert_bits(torch, got, reference(bt, boxes, size, 1, [1, 0], *IMAGENET, "float16", reduce=reduce), "model layer")
    plain = m.decode_batch_async(lists, dev, tensor=dict(size=(64, 64), origin=([5, 7], [9, 11])))
    m.codec().check()
    want = np.stack([r[:, y:y + 64, x:x + 64] for r, y, x in zip(rgbs, (5, 7), (9, 11))]).astype(np.float32) / np.float32(255)
    assert_bits(torch, plain, want, "tensor= without boxes")
    with pytest.raises(TypeError):
        m.decode_batch_async(lists, dev, tensor=dict(size=size, boxes=boxes, origin=([0, 0], [0, 0])))
