"""GPU tests far from the start of every buffer (run with -m gpu on an MI355X): offsets past 2^31 and 2^32, in bytes and in elements, in every
buffer the kernels index, and the largest image the format takes (8160x8160).  The rest of the suite stays within ~1.3 GiB of a buffer's base;
the library admits any batch of images up to 8160x8160, indexes with `long` almost everywhere and keeps a few deliberate 32-bit quantities
whose bounds are argued in comments ("Size limits", lists them): truncating one of them, or narrowing a `long`, fails here.

References: plain torch integer arithmetic on the device, in chunks (the lift); the SAME entry point called with B = 1 on single images of the
batch (the aliasing check: an image far into a buffer must get what it gets alone); and the CPU oracle on crops -- the band CNN is local, so a
crop's band grids are bit-equal to the image's from margin 2 inwards (helpers.crop_windows; tests/test_large_cpu.py holds that rule on the oracle).

Every test adds up what it needs (the library's size queries plus its own tensors), skips -- naming need and free -- only if the device has
less than that plus 2 GiB free, stays at or below 64 GiB, and prints its wall time and torch.cuda.max_memory_allocated() (run with -s)."""
import contextlib
import ctypes as C
import gc
import time

import numpy as np
import pytest

from conftest import load_state_dict
from helpers import crop_windows
from llicti_amd.codec import _ptr

pytestmark = pytest.mark.gpu

GIB = 1 << 30
CAP = 64 * GIB
OFFS = {0: (1, 1), 1: (0, 1), 2: (1, 0)}          # (oi, oj) of a band's target sub-band


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture()
def codec(torch_mod):
    """A fresh HipCodec per test (its cached workspace is the test's largest allocation), closed and released afterwards."""
    from llicti_amd.codec import HipCodec
    made = []

    def get(wname="rand1337"):
        c = HipCodec("cuda:0")
        c.load_state_dict(load_state_dict(wname))
        made.append(c)
        return c
    yield get
    for c in made:
        c._ws = None
        c.close()
    del made[:]
    gc.collect()
    torch_mod.cuda.empty_cache()


@contextlib.contextmanager
def large(torch, name, need, crossed):
    """need: bytes the test adds up for itself; crossed: what passes 2^31 / 2^32 (printed with the measurements)."""
    assert need <= CAP, f"{name}: needs {need / GIB:.1f} GiB, over the {CAP // GIB} GiB cap of a test"
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < need + 2 * GIB:
        pytest.skip(f"{name}: needs {need / GIB:.1f} GiB + 2 GiB, the device has {free / GIB:.1f} GiB free")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    dt, peak = time.perf_counter() - t0, torch.cuda.max_memory_allocated()
    print(f"\nLARGE {name}: wall {dt:.1f} s, peak {peak / GIB:.2f} GiB (added up beforehand: {need / GIB:.2f} GiB); {crossed}")
    assert peak <= CAP, (name, peak)


def noise(torch, shape, seed, lo=0, hi=256, chunk=32):
    """uint8 noise made ON THE DEVICE under a seeded generator, `chunk` leading entries at a time"""
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    out = torch.empty(shape, dtype=torch.uint8, device="cuda:0")
    for i in range(0, shape[0], chunk):
        out[i:i + chunk].random_(lo, hi, generator=g)
    return out


def used60(p64):
    """[B, 64, h, w] CNN outputs -> the 4 x 15 planes the kernel writes (the 16th of a head never is)"""
    B, _, h, w = p64.shape
    return p64.view(B, 4, 16, h, w)[:, :, :15]


def div255(torch, t):
    """t.float() / 255 as ONE correctly rounded fp32 division per element.  (Dividing a device tensor by a Python number multiplies by the
    reciprocal, which is not the same thing: the divisor is a device tensor.  numpy, on the images a test copies, is the authority.)"""
    return t.float() / torch.full((1,), 255.0, dtype=torch.float32, device=t.device)


def same_bits(torch, a, b):
    """float32 tensors equal as bit patterns (-0.0 and NaN included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def mm6_of(mm4):
    """device min/max words (minCo, minCg, maxCo, maxCg) -> the oracle's (minY, minCo, minCg, maxY, maxCo, maxCg); Y's range is fixed"""
    a = [int(v) for v in mm4]
    return np.array([0, a[0], a[1], 255, a[2], a[3]], np.int16)


# ------------------------------------------------------------------------------------------------ (a) lift / unlift / lift_train
def ycocg(torch, rgb):
    """YCoCg-R (Y - 127, Co, Cg) in plain integer arithmetic: uint8 [n, 3, H, W] -> (int16 [n, 3, H, W], int32 [n, 4] = min Co, min Cg, max Co, max Cg).
    `>>` on a signed tensor is arithmetic."""
    r, g, b = (rgb[:, k].to(torch.int32) for k in range(3))
    co = r - b
    t = b + (co >> 1)
    cg = g - t
    y = t + (cg >> 1) - 127
    mm = torch.stack([co.amin((1, 2)), cg.amin((1, 2)), co.amax((1, 2)), cg.amax((1, 2))], 1).to(torch.int32)
    return torch.stack([y, co, cg], 1).to(torch.int16), mm


EXTREMES = ((255, -1, 0), (0, -1, 255), (0, 255, 0), (255, 0, 255))      # -> Co = 255, Co = -255, Cg = 255, Cg = -255; -1: the pixel's green stays


@pytest.mark.parametrize("H,W", [(1536, 1024), (1535, 1023)])
def test_lift_unlift_past_4gib(torch_mod, codec, H, W):
    """B = 1024: rgb is 4.8 GB (its last image starts past 2^32 BYTES), planes and fplanes pass 2^32 ELEMENTS (9.7 and 19.3 GB).  1535x1023: the plane
    is no multiple of 4, so the lift takes its scalar path.  Pixel values lie in [64, 192) except ONE pixel per image of an extreme colour, at a place
    that depends on the image -- the first pixel of image 0, the last of image B - 1, the pixel in front of the last row's W % 4 tail -- which alone
    decides one of the image's four min/max words."""
    from oracle import oracle as orc
    torch = torch_mod
    B, plane = 1024, H * W
    px = B * 3 * plane
    need = px * (1 + 2 + 4 + 4) + 6 * GIB           # rgb, planes, fplanes (then the training planes in their place), the unlifted pixels; chunked references
    with large(torch, f"lift {B}x{H}x{W}", need, f"rgb {px / 1e9:.2f} GB = {px / 2**32:.2f} x 2^32 bytes; planes / fplanes {px / 2**32:.2f} x 2^32 elements, "
               f"{2 * px / 1e9:.1f} / {4 * px / 1e9:.1f} GB"):
        c = codec()
        rgb = noise(torch, (B, 3, H, W), 1000 + W, 64, 192)
        pos = [(b * 2654435761) % plane for b in range(B)]
        for b in range(B):
            if W % 4 and b % 8 == 5:
                pos[b] = (H - 1) * W + (W - W % 4 - 1)
        pos[0], pos[B - 1] = 0, plane - 1
        bidx = torch.arange(B, device="cuda:0")
        pos_d = torch.tensor(pos, device="cuda:0")
        col = torch.tensor([EXTREMES[b % 4] for b in range(B)], device="cuda:0")
        flat = rgb.view(B, 3, plane)
        green = flat[bidx, 1, pos_d].to(torch.int64)
        for k in range(3):
            flat[bidx, k, pos_d] = (torch.where(col[:, k] < 0, green, col[:, k]) if k == 1 else col[:, k]).to(torch.uint8)
        planes, fplanes, mm = c.lift(rgb)
        CH = 32
        for i in range(0, B, CH):
            p_ref, mm_ref = ycocg(torch, rgb[i:i + CH])
            assert torch.equal(planes[i:i + CH], p_ref), ("planes", i)
            assert torch.equal(mm[i:i + CH], mm_ref), ("min/max", i)
            assert same_bits(torch, fplanes[i:i + CH], div255(torch, p_ref)), ("fplanes", i)
            del p_ref
        mm_h = mm.cpu().numpy()
        for b in range(B):                            # (the extreme pixel decided its word: the inputs are what the docstring says)
            assert mm_h[b, (2, 0, 3, 1)[b % 4]] == (255, -255, 255, -255)[b % 4], b
        five = (0, 1, B // 2, B - 2, B - 1)
        for b in five:                                # numpy is the authority on the division
            assert np.array_equal(fplanes[b].cpu().numpy(), planes[b].cpu().numpy().astype(np.float32) / np.float32(255)), b
        back = c.unlift(planes)
        for i in range(0, B, 128):
            assert torch.equal(back[i:i + 128], rgb[i:i + 128]), ("unlift", i)
        del back, fplanes, planes
        torch.cuda.empty_cache()
        ftrain = c.lift_train(rgb)
        for b in five:
            assert np.array_equal(ftrain[b].cpu().numpy(), orc.lift_train(rgb[b].cpu().numpy())), ("lift_train", b)
        c.check()
        del ftrain, rgb, flat


# ------------------------------------------------------------------------------------------------ crops against the oracle
class Crop:
    """One crop of one image of a batch, with what the oracle says about it: its planes (host), per (level, band) the oracle's band_params."""

    def __init__(self, orc, W_o, planes_img, y0, x0, ch, cw):
        self.orc, self.W_o = orc, W_o
        self.y0, self.x0 = y0, x0
        self.H, self.W = planes_img.shape[-2:]
        crop, self.wins = crop_windows(planes_img, y0, x0, ch, cw, margin=2)
        self.planes = np.ascontiguousarray(crop.cpu().numpy())
        self.Hc, self.Wc = self.planes.shape[1:]
        self._par = {}

    def par(self, lvl, band):
        if (lvl, band) not in self._par:
            self._par[(lvl, band)] = self.orc.band_params(self.planes, lvl, band, self.W_o)
        return self._par[(lvl, band)]

    def grid(self, lvl):
        """(row offset, column offset, rows, columns) of the crop's band grid inside the image's"""
        fr, fc, cr, cc = self.wins[lvl]
        gh, gw = self.par(lvl, 0).shape[:2]
        return fr.start - cr.start, fc.start - cc.start, gh, gw

    def coded_window(self, lvl, band):
        """the window in CODED positions: (rows, columns of the image's coded crop; rows, columns of the crop's; (hc, wc) of the image, of the crop)"""
        from llicti_amd._lib import level_geom
        fr, fc, cr, cc = self.wins[lvl]
        *_, hf, wf = level_geom(self.H, self.W, lvl, band)
        *_, hcc, wcc = level_geom(self.Hc, self.Wc, lvl, band)
        oy, ox = fr.start - cr.start, fc.start - cc.start
        assert hf - oy == hcc and wf - ox == wcc or (self.y0 == 0 and self.x0 == 0)
        r1, c1 = min(cr.stop, hcc), min(cc.stop, wcc)
        return slice(fr.start, oy + r1), slice(fc.start, ox + c1), slice(cr.start, r1), slice(cc.start, c1), (hf, wf), (hcc, wcc)


def check_params_vs_oracle(c, p64_img, crop, lvl, band, what):
    """p64_img: [1, 64, h, w] of the crop's image"""
    fr, fc, cr, cc = crop.wins[lvl]
    got = np.ascontiguousarray(c.params60(p64_img)[0, fr, fc].cpu().numpy())
    ref = np.ascontiguousarray(crop.par(lvl, band)[cr, cc])
    assert got.shape == ref.shape and got.size > 0
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (what, "band_params vs oracle", lvl, band, float(np.abs(got - ref).max()))


def check_pairs_vs_oracle(pairs_img, mm4, crop, lvl, band, what):
    """pairs_img: int32 [3, hc * wc] of the crop's image (device); the oracle codes the crop with the IMAGE's min/max"""
    rf, cf, rc, cc, (hf, wf), (hcc, wcc) = crop.coded_window(lvl, band)
    mm6 = mm6_of(mm4)
    got = pairs_img.reshape(3, hf, wf)[:, rf, cf].cpu().numpy().view(np.uint32)
    for clr in range(3):
        clow, chigh, _ = crop.orc.stream_pairs(crop.planes, mm6, lvl, band, clr, crop.par(lvl, band))
        assert clow.size == hcc * wcc
        assert np.array_equal(got[clr] & 0xFFFF, clow.reshape(hcc, wcc)[rc, cc]), (what, "pairs (low) vs oracle", lvl, band, clr)
        assert np.array_equal(got[clr] >> 16, (chigh & 0xFFFF).reshape(hcc, wcc)[rc, cc]), (what, "pairs (high) vs oracle", lvl, band, clr)


def check_rows_vs_oracle(tab_img, mm4, crop, lvl, band, clr, what):
    """tab_img: int16 [hc * wc, 512] of the crop's image (device): the rows of the window against orc.cdf_rows with the IMAGE's min/max"""
    rf, cf, rc, cc, (hf, wf), _ = crop.coded_window(lvl, band)
    mm6 = mm6_of(mm4)
    minv, maxv = (-127, 128) if clr == 0 else (int(mm6[clr]), int(mm6[3 + clr]))
    Lp = maxv - minv + 2
    got = tab_img.view(hf, wf, 512)[rf, cf].cpu().numpy().view(np.uint16).reshape(-1, 512)
    oi, oj = OFFS[band]
    ii, jj = np.meshgrid(np.arange(rc.start, rc.stop), np.arange(cc.start, cc.stop), indexing="ij")
    R, Cc = ((2 * ii + oi) << lvl).ravel(), ((2 * jj + oj) << lvl).ravel()
    tg = crop.planes[:, R, Cc].astype(np.float32) / np.float32(255)
    rows = crop.orc.cdf_rows(crop.par(lvl, band)[rc, cc].reshape(-1, 60), clr, tg[0], tg[1], minv, maxv)
    assert got.shape[0] == rows.shape[0] and rows.shape[0] > 0
    assert np.array_equal(got[:, :Lp], rows), (what, "table rows vs oracle", lvl, band, clr)
    assert (got[:, Lp:] == 0xFFFF).all()


# ------------------------------------------------------------------------------------------------ (b) CNN, tables, pairs, self-information
def test_cnn_tables_pairs_selfinfo_past_4gib(torch_mod, codec, oracle_weights):
    """B = 928 of 512x768: fplanes are 4.4 GB, the level-0 CNN outputs 23 GB = 5.8 G elements, the level-2 table rows (row_stride 512) 5.8 GB.
    band_params and cdf_pairs at all 5 levels x 3 bands, cdf_tables at level 2, selfinfo on the training path's planes: for images
    {0, 1, B/2, B-2, B-1} every output is bit-equal to the same entry point called with B = 1 on that image alone; the bottom-right crop of image
    B - 1 and the top-left 192x192 of image 0 are bit-equal to the oracle (params, pairs, table rows) and selfinfo there is within
    ref64.selfinfo64's tolerance.  Level 0, band 2 once more with cnn_tile_rows = 4."""
    import ref64
    from llicti_amd._lib import level_geom
    from oracle import oracle as orc
    torch = torch_mod
    B, H, W = 928, 512, 768
    px = B * 3 * H * W
    par0 = B * 64 * (H // 2) * (W // 2) * 4
    tab2 = B * (H // 8) * (W // 8) * 512 * 2
    need = px * (1 + 2 + 4 + 4) + par0 + max(px, tab2) + 2 * GIB
    with large(torch, f"kernel level {B}x{H}x{W}", need, f"fplanes {4 * px / 1e9:.2f} GB; level-0 params {par0 / 1e9:.1f} GB = {par0 / 4 / 2**32:.2f} x 2^32 elements; "
               f"level-2 tables {tab2 / 1e9:.2f} GB; level-0 pairs {px * 4 / 4 / 1e9:.2f} GB"):
        c = codec()
        W_o = oracle_weights("rand1337")
        rgb = noise(torch, (B, 3, H, W), 77)
        planes, fplanes, mm = c.lift(rgb)
        mm_h = mm.cpu().numpy()
        five = (0, 1, B // 2, B - 2, B - 1)
        crops = {B - 1: Crop(orc, W_o, planes[B - 1], (H - 192) // 32 * 32, (W - 192) // 32 * 32, None, None), 0: Crop(orc, W_o, planes[0], 0, 0, 192, 192)}

        def check_params(p, lvl, band, what):
            for b in five:
                one = c.band_params(fplanes[b:b + 1], lvl, band)
                assert same_bits(torch, used60(p[b:b + 1]), used60(one)), (what, "band_params vs B = 1", lvl, band, b)
            for b, crop in crops.items():
                check_params_vs_oracle(c, p[b:b + 1], crop, lvl, band, what)

        for lvl in range(5):
            for band in range(3):
                p = c.band_params(fplanes, lvl, band)
                check_params(p, lvl, band, "automatic tile form")
                pairs = c.cdf_pairs(planes, p, mm, lvl, band)                     # [3, B, hc * wc]
                for b in five:
                    one = c.cdf_pairs(planes[b:b + 1], p[b:b + 1], mm[b:b + 1], lvl, band)
                    assert torch.equal(pairs[:, b], one[:, 0]), ("cdf_pairs vs B = 1", lvl, band, b)
                for b, crop in crops.items():
                    check_pairs_vs_oracle(pairs[:, b], mm_h[b], crop, lvl, band, f"image {b}")
                del pairs
                if lvl == 2:
                    for clr in range(3):
                        tab = c.cdf_tables(planes, p, mm, lvl, band, clr, row_stride=512)      # [B, hc * wc, 512]
                        assert tab.numel() * 2 > 1 << 32
                        for b in five:
                            one = c.cdf_tables(planes[b:b + 1], p[b:b + 1], mm[b:b + 1], lvl, band, clr, row_stride=512)
                            assert torch.equal(tab[b], one[0]), ("cdf_tables vs B = 1", lvl, band, clr, b)
                        for b, crop in crops.items():
                            check_rows_vs_oracle(tab[b], mm_h[b], crop, lvl, band, clr, f"image {b}")
                        del tab, one
                del p
        try:
            c.set_tuning("cnn_tile_rows", 4)
            p = c.band_params(fplanes, 0, 2)
            c.set_tuning("cnn_tile_rows", 0)
            check_params(p, 0, 2, "4-row tiles")            # (the B = 1 calls run the automatic form: the forms agree bit for bit)
            del p
        finally:
            c.set_tuning("cnn_tile_rows", 0)
        del fplanes
        torch.cuda.empty_cache()
        # the training path: float lift -> CNN -> self-information
        ftrain = c.lift_train(rgb)
        ft_h = {b: ftrain[b].cpu().numpy() for b in crops}
        worst = 0.0
        for lvl in range(5):
            for band in range(3):
                p = c.band_params(ftrain, lvl, band)
                si = c.selfinfo(ftrain, p, lvl, band)                           # [B, 3, h, w]
                for b in five:
                    one = c.selfinfo(ftrain[b:b + 1], p[b:b + 1], lvl, band)
                    assert same_bits(torch, si[b:b + 1], one), ("selfinfo vs B = 1", lvl, band, b)
                for b, crop in crops.items():
                    oy, ox, gh, gw = crop.grid(lvl)
                    fp_crop = np.ascontiguousarray(ft_h[b][:, crop.y0:crop.y0 + crop.Hc, crop.x0:crop.x0 + crop.Wc])
                    par = np.ascontiguousarray(c.params60(p[b:b + 1])[0, oy:oy + gh, ox:ox + gw].cpu().numpy())
                    ref, tol = ref64.selfinfo64(fp_crop, lvl, band, par)
                    got = si[b, :, oy:oy + gh, ox:ox + gw].cpu().numpy()
                    q = float((np.abs(got - ref) / tol).max())
                    assert q <= 1.0, ("selfinfo vs float64", lvl, band, b, q)
                    worst = max(worst, q)
                del p, si
        print(f"selfinfo: largest |kernel - float64| / tolerance on the crops: {worst:.3g}")
        c.check()
        del ftrain, planes, rgb


# ------------------------------------------------------------------------------------------------ (c) whole-batch calls
CB, CH_, CW_ = 3712, 256, 384


def lists_of(cont, seg, b):
    from llicti_amd.codec import container_to_bytestream_list
    return container_to_bytestream_list(cont[b].cpu().numpy(), seg[b].cpu().numpy())


def batch_need(c, Hs, Ws, mode, extra):
    """workspace (the library's size query; nothing is allocated) + containers + what the test holds itself"""
    B = len(Hs)
    one, per = c._modes_arg(mode, B)
    m = np.full(B, one, dtype=np.int32) if per is None else per
    Ha, Wa = np.ascontiguousarray(Hs, dtype=np.int32), np.ascontiguousarray(Ws, dtype=np.int32)
    ws = int(c.L.llicti_workspace_bytes_ctx(c.ctx, B, _ptr(Ha), _ptr(Wa), _ptr(m), B))
    assert ws > 0
    stride = max(c.max_container_bytes(int(h), int(w)) for h, w in set(zip(Hs, Ws)))
    return ws, ws + len(Hs) * stride + extra


@pytest.mark.parametrize("container", ["default", "rans4", "ac"])
def test_batch_roundtrip_past_4gib(torch_mod, codec, oracle_weights, container):
    """B = 3,712 of 256x384 noise in one encode and one decode: the workspace is ~40 GiB, the last image's fplanes start at 4.38 GB and the level-0
    CNN outputs are 5.8 G elements.  Lossless on a poisoned workspace, every image's status zero, and the containers of images {0, B/2, B-1} are the
    oracle's byte for byte."""
    from bench import default_container
    from llicti_amd.codec import mode_of_name
    from oracle import oracle as orc
    torch = torch_mod
    B, H, W = CB, CH_, CW_
    name = default_container(H, W) if container == "default" else container
    mode = mode_of_name(name)
    c = codec()
    px = B * 3 * H * W
    ws, need = batch_need(c, [H] * B, [W] * B, mode, 2 * px + GIB)
    with large(torch, f"round trip {B}x{H}x{W} {name}", need, f"workspace {ws / GIB:.1f} GiB; fplanes {4 * px / 1e9:.2f} GB; level-0 params {B * 64 * (H // 2) * (W // 2) / 2**32:.2f} x 2^32 elements"):
        W_o = oracle_weights("rand1337")
        rgb = noise(torch, (B, 3, H, W), 5)
        cont, seg = c.encode(rgb, mode)
        c.check()
        modes = c.container_modes(cont)                 # (an "auto" encode picked every image's stream count: the headers say which)
        for b in (0, B // 2, B - 1):
            img = rgb[b].cpu().numpy()
            M = int("".join(ch for ch in name if ch.isdigit()) or 0)
            ref = orc.encode_image(img, W_o) if name == "ac" else orc.encode_image_rans(img, W_o, M, 2 if name[0] == "x" else 0, auto=name.startswith("xauto"))
            assert lists_of(cont, seg, b) == ref, (name, "container vs oracle", b)
        c.poison_workspace()
        rec = c.decode_v(cont, seg, [H] * B, [W] * B, modes)
        c.check()
        assert (c.image_status(B) == 0).all()
        assert torch.equal(rec.view(B, 3, H, W), rgb)
        del rec, cont, seg, rgb


def test_mixed_sizes_past_4gib(torch_mod, codec, oracle_weights):
    """The same pixel budget in sizes cycling (256x384, 250x391, 192x512) through encode_v / decode_v, each image in its own "auto" mode: the
    mixed-size (tile-list) form of every kernel, far into the buffers."""
    from llicti_amd.codec import auto_modes, image_streams
    from oracle import oracle as orc
    torch = torch_mod
    B = CB
    sizes = [((256, 384), (250, 391), (192, 512))[b % 3] for b in range(B)]
    Hs, Ws = [s[0] for s in sizes], [s[1] for s in sizes]
    modes = auto_modes(sizes)
    c = codec()
    offs, total = c.flat_offsets(Hs, Ws)
    ws, need = batch_need(c, Hs, Ws, modes, 2 * total + GIB)
    with large(torch, f"mixed sizes, {B} images", need, f"workspace {ws / GIB:.1f} GiB; fplanes {4 * total / 1e9:.2f} GB"):
        W_o = oracle_weights("rand1337")
        flat = noise(torch, (total // 4096 + 1, 4096), 6, chunk=8192).view(-1)[:total].contiguous()
        cont, seg = c.encode_v(flat, Hs, Ws, modes)
        c.check()
        got_modes = c.container_modes(cont)
        for b in (0, B // 2, B - 1):
            h, w = sizes[b]
            img = flat[int(offs[b]):int(offs[b]) + 3 * h * w].view(3, h, w).cpu().numpy()
            assert lists_of(cont, seg, b) == orc.encode_image_rans(img, W_o, image_streams(h, w), 2, auto=True), ("container vs oracle", b)
        c.poison_workspace()
        rec = c.decode_v(cont, seg, Hs, Ws, got_modes)
        c.check()
        assert (c.image_status(B) == 0).all()
        assert torch.equal(rec, flat)
        del rec, cont, seg, flat


def test_float_tensors_past_4gib(torch_mod, codec):
    """encode_f32's input and decode_tensor's float32 output of the equal-size batch are 4.4 GB each: encode_f32(x / 255) gives the uint8 call's
    containers, decode_tensor (full window, no normalisation) exactly u8.float() / 255; a 32x32 float16 window at every image's largest origin with
    ImageNet's mean / std is the CPU spec's (tests/test_hip_tensor.py) for images {0, B/2, B-1}."""
    from bench import default_container
    from llicti_amd.codec import mode_of_name
    from test_hip_tensor import spec
    torch = torch_mod
    B, H, W = CB, CH_, CW_
    mode = mode_of_name(default_container(H, W))
    c = codec()
    px = B * 3 * H * W
    ws, need1 = batch_need(c, [H] * B, [W] * B, mode, 0)
    need = need1 + (need1 - ws) + px * (1 + 4) + 3 * GIB       # a second set of containers; the pixels; x, which the decoded tensor then takes; chunked comparisons
    with large(torch, f"float tensors {B}x{H}x{W}", need, f"workspace {ws / GIB:.1f} GiB; float32 input and output {4 * px / 1e9:.2f} GB each"):
        u8 = noise(torch, (B, 3, H, W), 8)
        x = torch.empty((B, 3, H, W), dtype=torch.float32, device="cuda:0")
        for i in range(0, B, 256):
            x[i:i + 256] = div255(torch, u8[i:i + 256])
        cont, seg = c.encode(u8, mode)
        c.check()
        cont_f, seg_f = c.encode_f32(x.view(-1), [H] * B, [W] * B, mode)
        c.check()
        assert torch.equal(seg_f, seg)
        length = seg.sum(1)
        col = torch.arange(cont.shape[1], device="cuda:0")
        for i in range(0, B, 256):
            keep = col[None, :] < length[i:i + 256, None]
            assert torch.equal(cont_f[i:i + 256][keep], cont[i:i + 256][keep]), ("encode_f32 containers", i)
        del cont_f, seg_f, keep
        modes = c.container_modes(cont)
        c.poison_workspace()
        out = c.decode_tensor(cont, seg, [H] * B, [W] * B, modes, size=(H, W), out=x)      # (into x's 4.4 GB: the input is no longer needed)
        c.check()
        assert (c.image_status(B) == 0).all()
        for i in range(0, B, 256):
            assert same_bits(torch, out[i:i + 256], div255(torch, u8[i:i + 256])), ("decode_tensor", i)
        for b in (0, B // 2, B - 1):                  # (the CPU's division is the authority)
            assert torch.equal(out[b].cpu(), spec(torch, u8[b].cpu())), ("decode_tensor vs the CPU spec", b)
        del out, x
        mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
        c.poison_workspace()
        win = c.decode_tensor(cont, seg, [H] * B, [W] * B, modes, size=(32, 32), dtype=torch.float16, origin=([H - 32] * B, [W - 32] * B), mean=mean, std=std)
        c.check()
        assert (c.image_status(B) == 0).all()
        for b in (0, B // 2, B - 1):
            assert torch.equal(win[b].cpu(), spec(torch, u8[b, :, H - 32:, W - 32:].cpu(), mean, std, torch.float16)), ("window", b)
        del win, cont, seg, u8


# ------------------------------------------------------------------------------------------------ (d) the largest legal image
@pytest.mark.parametrize("H,W", [(8160, 8160), (8159, 8157)])
def test_largest_image_kernels(torch_mod, codec, oracle_weights, H, W):
    """One image of the largest size (and its odd neighbour: a pad at every level, W % 4 != 0): the level-0 CNN outputs are 4.26 GB INSIDE one image,
    so (head 16 + 4 q) npos + i w + j passes 2^31 bytes and ends 34 MB short of 2^32 (63 used planes of 66.6 MB).  lift -> band_params at all levels and bands -> cdf_pairs; the bottom-right crop and the
    top-left 192x192 against the oracle, bit for bit."""
    from oracle import oracle as orc
    torch = torch_mod
    px = 3 * H * W
    par0 = 64 * ((H + 1) // 2) * ((W + 1) // 2) * 4
    need = px * (1 + 2 + 4) + par0 + px * 4 + 4 * GIB        # rgb, planes, fplanes; level-0 params and pairs; the integer reference of the lift
    with large(torch, f"kernel level 1x{H}x{W}", need, f"level-0 params of ONE image {par0 / 1e9:.2f} GB = {par0 / 2**32:.3f} x 2^32 bytes"):
        c = codec()
        W_o = oracle_weights("rand1337")
        rgb = noise(torch, (3, H, W), 90 + (H & 1), chunk=1).view(1, 3, H, W)
        planes, fplanes, mm = c.lift(rgb)
        p_ref, mm_ref = ycocg(torch, rgb)
        assert torch.equal(planes, p_ref) and torch.equal(mm, mm_ref)
        del p_ref
        mm_h = mm.cpu().numpy()
        crops = [Crop(orc, W_o, planes[0], (H - 192) // 32 * 32, (W - 192) // 32 * 32, None, None), Crop(orc, W_o, planes[0], 0, 0, 192, 192)]
        for lvl in range(5):
            for band in range(3):
                p = c.band_params(fplanes, lvl, band)
                pairs = c.cdf_pairs(planes, p, mm, lvl, band)
                for k, crop in enumerate(crops):
                    check_params_vs_oracle(c, p, crop, lvl, band, ("bottom-right", "top-left")[k])
                    check_pairs_vs_oracle(pairs[:, 0], mm_h[0], crop, lvl, band, ("bottom-right", "top-left")[k])
                del p, pairs
        c.check()
        del planes, fplanes, rgb


@pytest.mark.parametrize("H,W", [(8160, 8160), (8159, 8157)])
def test_largest_image_roundtrip(torch_mod, codec, H, W):
    """Encode in MODE_RANS(2, wide=2) -- the fewest streams the bound on a stream's bits admits: about 1.35 Gbit per stream, past 2^30 -- and in
    what container "auto" gives the size; decode on a poisoned workspace; the header reads back.  ONE stream is refused with LLICTI_EINVAL before
    anything is launched: no plan is built or looked up, and the next check() is clean."""
    from llicti_amd import _lib
    from llicti_amd.codec import MODE_RANS, NSEG, _stream_ptr, auto_modes, header_dims, mode_of_header
    torch = torch_mod
    px = 3 * H * W
    c = codec()
    few, auto = MODE_RANS(2, wide=2), auto_modes([(H, W)])[0]
    ws, need = batch_need(c, [H], [W], few, 0)
    ws2, need2 = batch_need(c, [H], [W], auto, 0)
    ws, need = max(ws, ws2), max(need, need2) + max(ws, ws2) // 4 + 2 * px + GIB      # (the codec grows its cached workspace by a quarter when a second mode needs more)
    with large(torch, f"round trip 1x{H}x{W}", need, f"workspace {ws / GIB:.1f} GiB; a stream of the 2-stream container holds {px / 2 / 1e6:.0f} M symbols of up to 16 bits"):
        rgb = noise(torch, (3, H, W), 190 + (H & 1), chunk=1).view(1, 3, H, W)
        for mode in (few, auto):
            cont, seg = c.encode(rgb, mode)
            c.check()
            if mode == few:
                per_stream = seg[0, 4:6].cpu().numpy().astype(np.int64) * 8
                print(f"\n{H}x{W} in 2 xwide streams: {per_stream[0] / 1e9:.3f} and {per_stream[1] / 1e9:.3f} Gbit")
                assert per_stream.min() > 1 << 30                     # (the test is about bit positions past 2^30)
            hdr = bytes(cont[0, :17].cpu().numpy())
            named = C.c_int()
            _lib.check(c.L.llicti_header_mode((C.c_uint8 * 17).from_buffer_copy(hdr), C.byref(named)))
            assert header_dims(hdr) == (H, W) and named.value == mode and mode_of_header(hdr) == mode
            c.poison_workspace()
            rec = c.decode(cont, seg, H, W, mode)
            c.check()
            assert (c.image_status(1) == 0).all()
            assert torch.equal(rec, rgb)
            del rec
        # one stream, every lane kind: refused on the host.  (Never run "to see": a stream's bit cursor would pass 2^31.)
        ws_t = c.workspace(1, H, W, few)
        out_seg = torch.zeros((1, NSEG), dtype=torch.int32, device="cuda:0")
        names = ("plan_builds", "plan_hits", "device_allocs", "device_syncs")
        before = [c.counter(n) for n in names]
        for one in (MODE_RANS(1), MODE_RANS(1, wide=1), MODE_RANS(1, wide=2)):
            assert int(c.L.llicti_workspace_bytes(1, H, W, one)) == 0
            rc = c.L.llicti_encode_images(c.ctx, _ptr(rgb), 1, H, W, one, _ptr(ws_t), ws_t.numel(), _ptr(cont), cont.shape[1], _ptr(out_seg), _stream_ptr(c.device))
            assert rc == _lib.EINVAL, (hex(one), rc)
            msg = c.L.llicti_last_error().decode()
            assert f"image 0 is {W}x{H}" in msg and "smallest count that fits is 2" in msg, msg
            rc = c.L.llicti_decode_images(c.ctx, _ptr(cont), cont.shape[1], _ptr(seg), 1, H, W, one, _ptr(ws_t), ws_t.numel(), _ptr(rgb), _stream_ptr(c.device))
            assert rc == _lib.EINVAL, (hex(one), rc)
        assert [c.counter(n) for n in names] == before
        c.check()
        assert int(out_seg.abs().sum()) == 0
        del cont, seg, rgb, ws_t
