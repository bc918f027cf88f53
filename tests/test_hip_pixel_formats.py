"""Interleaved, pitched 8-bit pixel buffers on the GPU (run with -m gpu on an MI355X): llicti_encode_images_px / llicti_decode_images_px read and
write RGB8 / BGR8 / RGBA8 / BGRA8 windows of the caller's buffer.  A container is a function of the pixel values alone, so every check is EXACT and
the yardstick is the planar path (itself pinned to the oracle) on the same values: same container bytes and segment lengths on the way in, the
expected interleaving -- and not one byte outside the windows -- on the way out.  The shapes are the smallest that reach every form of the row
walk: 32x32 (the minimum), 33x35 and 67x93 (W % 4 != 0: the byte-wise row tail, rows that start at odd bytes when packed tightly, both pad flags),
64x96 (short4 / float4 planes, dword pixels), and crops of a 96x128 canvas."""
import numpy as np
import pytest

from conftest import load_state_dict
from helpers import make_image

pytestmark = pytest.mark.gpu

FORMATS = ["rgb", "bgr", "rgba", "bgra"]
SHAPES = [(32, 32), (33, 35), (67, 93), (64, 96)]
MODELS = [(5, "ac"), (5, "xrans2"), (5, "auto"), (2, "ac"), (2, "xrans2")]      # (levels, container): config A, config B
CANVAS = (96, 128)
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


def _mode(name, sizes, nlev):
    from llicti_amd.codec import auto_modes, mode_of_name
    if name != "auto":
        return mode_of_name(name)
    modes = auto_modes(sizes, nlev)
    return modes[0] if all(m == modes[0] for m in modes) else modes


def _bpp(fmt):
    return 4 if fmt.endswith("a") else 3


def interleave(rgb, fmt, alpha=None):
    """uint8 [3, H, W] -> uint8 [H, W, bpp] in the format's byte order; alpha: the fourth byte (an array or a value; default: a pattern)."""
    H, W = rgb.shape[1:]
    out = np.empty((H, W, _bpp(fmt)), dtype=np.uint8)
    order = (2, 1, 0) if fmt.startswith("bgr") else (0, 1, 2)
    for k, ch in enumerate(order):
        out[:, :, k] = rgb[ch]
    if _bpp(fmt) == 4:
        out[:, :, 3] = (np.arange(H * W, dtype=np.uint32).reshape(H, W) * 37 + 11).astype(np.uint8) if alpha is None else alpha
    return out


def place(windows, fill_seed=0, fill=None):
    """windows: [(hwc array or None, offset, pitch)] -> flat uint8 host buffer with every window's rows at offset + i * pitch; the other bytes are
    noise (an encoder must not care) or `fill`.  None: the window's bytes are left as filled (a decode target)."""
    end = 0
    for a, off, pitch, (h, w, bpp) in windows:
        end = max(end, off + (h - 1) * pitch + w * bpp)
    total = end + 61
    buf = np.random.default_rng(fill_seed).integers(0, 256, total, dtype=np.uint8) if fill is None else np.full(total, fill, dtype=np.uint8)
    for a, off, pitch, (h, w, bpp) in windows:
        if a is None:
            continue
        for i in range(h):
            buf[off + i * pitch: off + i * pitch + w * bpp] = a[i].reshape(-1)
    return buf


def window_mask(total, windows):
    m = np.zeros(total, dtype=bool)
    for _, off, pitch, (h, w, bpp) in windows:
        for i in range(h):
            m[off + i * pitch: off + i * pitch + w * bpp] = True
    return m


def read_window(buf, off, pitch, h, w, bpp):
    return np.stack([buf[off + i * pitch: off + i * pitch + w * bpp].reshape(w, bpp) for i in range(h)])


_PLANAR = {}


def planar(torch, c, nlev, rgb, name, mode=None):
    """The yardstick, computed once per (model, image, container): the planar single-image encode -> (container bytes, seg_len row).
    mode: the image's encoder mode where the container's name does not say it (container "auto" gives the images of one call one lane kind)."""
    key = (nlev, name if mode is None else mode, rgb.shape, rgb.tobytes())
    if key not in _PLANAR:
        H, W = rgb.shape[1:]
        mode = _mode(name, [(H, W)], nlev) if mode is None else mode
        cont, seg = c.encode(_dev(torch, rgb[None]), mode=mode)
        c.check()
        seg = seg[0].cpu().numpy().copy()
        _PLANAR[key] = (cont[0, :int(seg.sum())].cpu().numpy().copy(), seg)
    return _PLANAR[key]


def encode_px(torch, c, nlev, buf, fmt, sizes, name, offs, pitches):
    Hs, Ws = [h for h, _ in sizes], [w for _, w in sizes]
    mode = _mode(name, sizes, nlev)
    cont, seg = c.encode_px(_dev(torch, buf), Hs, Ws, mode, fmt, px_off=offs, pitch=pitches)
    c.check()
    seg = seg.cpu().numpy()
    return [cont[b, :int(seg[b].sum())].cpu().numpy() for b in range(len(sizes))], seg, cont


def assert_same_container(got, seg, want, what):
    assert np.array_equal(seg, want[1]), (what, "seg_len differs", seg[:8], want[1][:8])
    assert np.array_equal(got, want[0]), (what, "container bytes differ")


# ------------------------------------------------------------------------------------------------ same bytes as the planar path
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("nlev,name", MODELS)
def test_same_container_as_planar(torch_mod, codecs, nlev, name, H, W):
    """Every format, tightly packed (None arrays; W % 4 != 0: rows at odd bytes) and with the pitch rounded up to a multiple of 4 at an aligned
    offset (dword pixels next to a byte-wise row tail): the container and seg_len of the planar encode of the same pixel values."""
    torch = torch_mod
    c = codecs(nlev)
    rgb = make_image("smooth" if (H + W) % 2 else "noise", H, W, 300 + H + W)
    want = planar(torch, c, nlev, rgb, name)
    for fmt in FORMATS:
        bpp = _bpp(fmt)
        a = interleave(rgb, fmt)
        got, seg, _ = encode_px(torch, c, nlev, a.reshape(-1), fmt, [(H, W)], name, None, None)
        assert_same_container(got[0], seg[0], want, (fmt, "tight"))
        pitch = (W * bpp + 3) // 4 * 4 + 8
        buf = place([(a, 16, pitch, (H, W, bpp))], fill_seed=H)
        got, seg, _ = encode_px(torch, c, nlev, buf, fmt, [(H, W)], name, [16], [pitch])
        assert_same_container(got[0], seg[0], want, (fmt, "pitched"))


def test_against_the_oracle_directly(torch_mod, codecs, oracle_weights):
    """One image, BGRA at an odd offset, against the CPU oracle itself (not through the planar path): reference format and xwide streams."""
    torch = torch_mod
    from oracle import oracle as orc
    from llicti_amd.codec import container_to_bytestream_list
    c = codecs(5)
    rgb = make_image("smooth", 67, 93, 77)
    W_o = oracle_weights("trainedlike")
    buf = place([(interleave(rgb, "bgra"), 3, 93 * 4 + 1, (67, 93, 4))])
    for name, ref in (("ac", lambda: orc.encode_image(rgb, W_o)), ("xrans2", lambda: orc.encode_image_rans(rgb, W_o, 2, 2))):
        _, seg, cont = encode_px(torch, c, 5, buf, "bgra", [(67, 93)], name, [3], [93 * 4 + 1])
        assert container_to_bytestream_list(cont[0].cpu().numpy(), seg[0]) == ref(), name


# ------------------------------------------------------------------------------------------------ both forms of the row walk in one call
def _three_windows(fmt, seed):
    """A tight 4-byte-aligned 64x96 frame, a 33x35 frame with its pitch padded to 256 bytes, and a 67x93 crop that starts at an ODD byte inside a
    96x128 canvas (the canvas's pitch) -> (planar images, windows for place())."""
    bpp = _bpp(fmt)
    rgbs = [make_image("smooth", 64, 96, seed), make_image("noise", 33, 35, seed + 1), make_image("smooth", 67, 93, seed + 2)]
    cpitch = CANVAS[1] * bpp
    base = 64 * 96 * bpp + 33 * 256 + 64
    crop = base + 5 * cpitch + 3 * bpp
    if crop % 2 == 0:
        base += 1
        crop += 1
    wins = [(interleave(rgbs[0], fmt), 0, 96 * bpp, (64, 96, bpp)),
            (interleave(rgbs[1], fmt), 64 * 96 * bpp, 256, (33, 35, bpp)),
            (interleave(rgbs[2], fmt), crop, cpitch, (67, 93, bpp))]
    assert wins[0][1] % 4 == 0 and wins[1][1] % 4 == 0 and crop % 2 == 1 and crop + 66 * cpitch + 93 * bpp <= base + CANVAS[0] * cpitch
    return rgbs, wins


@pytest.mark.parametrize("name", ["xrans2", "auto"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_aligned_padded_and_odd_crop_in_one_call(torch_mod, codecs, fmt, name):
    torch = torch_mod
    c = codecs(5)
    rgbs, wins = _three_windows(fmt, 500)
    sizes = [r.shape[1:] for r in rgbs]
    modes = _mode(name, sizes, 5)                       # ("auto": what the CALL gives each image -- one lane kind for all three)
    got, seg, _ = encode_px(torch, c, 5, place(wins), fmt, sizes, name, [w[1] for w in wins], [w[2] for w in wins])
    for b, rgb in enumerate(rgbs):
        want = planar(torch, c, 5, rgb, name, mode=modes[b] if isinstance(modes, list) else modes)
        assert_same_container(got[b], seg[b], want, (fmt, name, b))


# ------------------------------------------------------------------------------------------------ decode into a canvas
@pytest.mark.parametrize("nlev,name,sizes", [(5, "xrans2", [(64, 96), (67, 93)]), (5, "ac", [(64, 96), (64, 96)]), (2, "xrans2", [(64, 96), (67, 93)])])
def test_decode_into_poisoned_canvas(torch_mod, codecs, nlev, name, sizes):
    """Two windows in one call -- an aligned one with padded pitch, and a crop at an odd byte of a canvas -- into a buffer of 0xA5, at reduce 0, 1
    and the model's maximum, every format: inside the windows the expected interleaving of full[::2^r, ::2^r] with alpha 255, everywhere else
    (pitch padding, the bytes between a row's end and the next row, the rest of the canvas) still 0xA5."""
    torch = torch_mod
    from llicti_amd.codec import reduced_dims
    c = codecs(nlev)
    rgbs = [make_image(("smooth", "noise")[i], h, w, 40 + i) for i, (h, w) in enumerate(sizes)]
    Hs, Ws = [h for h, _ in sizes], [w for _, w in sizes]
    mode = _mode(name, sizes, nlev)
    if len(set(sizes)) == 1:
        cont, seg = c.encode(_dev(torch, np.stack(rgbs)), mode=mode)
    else:
        cont, seg = c.encode_v(_dev(torch, np.concatenate([r.reshape(-1) for r in rgbs])), Hs, Ws, mode)
    c.check()
    for r in (0, 1, nlev):
        s = 1 << r
        dims = [reduced_dims(h, w, r) for h, w in sizes]
        for fmt in FORMATS:
            bpp = _bpp(fmt)
            p0 = (dims[0][1] * bpp + 3) // 4 * 4 + 12                     # aligned, padded
            cpitch = CANVAS[1] * bpp
            base = dims[0][0] * p0 + 32
            crop = base + 2 * cpitch + 1 * bpp
            crop += 1 - crop % 2                                          # an odd byte
            wins = [(None, 0, p0, (*dims[0], bpp)), (None, crop, cpitch, (*dims[1], bpp))]
            total = base + 1 + CANVAS[0] * cpitch
            out = torch.full((total,), POISON, dtype=torch.uint8, device="cuda:0")
            c.workspace_v(Hs, Ws, mode)
            c.poison_workspace(POISON)
            got = c.decode_px(cont, seg, Hs, Ws, mode, fmt, reduce=r, out=out, px_off=[0, crop], pitch=[p0, cpitch])
            c.check()
            assert (c.image_status(2) == 0).all()
            assert got.data_ptr() == out.data_ptr()
            host = out.cpu().numpy()
            for b, rgb in enumerate(rgbs):
                want = interleave(rgb[:, ::s, ::s], fmt, alpha=255)
                have = read_window(host, wins[b][1], wins[b][2], *wins[b][3])
                assert np.array_equal(have, want), (name, fmt, r, b)
            outside = ~window_mask(total, wins)
            assert (host[outside] == POISON).all(), (name, fmt, r, int((host[outside] != POISON).sum()))


# ------------------------------------------------------------------------------------------------ alpha, channel order
def test_alpha_is_ignored_and_bgr_is_rgb_swapped(torch_mod, codecs):
    torch = torch_mod
    c = codecs(5)
    rgb = make_image("smooth", 67, 93, 9)
    want = planar(torch, c, 5, rgb, "xrans2")
    for fmt in ("rgba", "bgra"):
        for alpha in (0, 255, None):
            got, seg, _ = encode_px(torch, c, 5, interleave(rgb, fmt, alpha).reshape(-1), fmt, [(67, 93)], "xrans2", None, None)
            assert_same_container(got[0], seg[0], want, (fmt, alpha))
    # the SAME bytes read as BGR are the image with red and blue swapped
    a = interleave(rgb, "rgb").reshape(-1)
    got, seg, _ = encode_px(torch, c, 5, a, "bgr", [(67, 93)], "xrans2", None, None)
    assert_same_container(got[0], seg[0], planar(torch, c, 5, np.ascontiguousarray(rgb[::-1]), "xrans2"), "rgb bytes as bgr")
    assert not np.array_equal(got[0], want[0])


# ------------------------------------------------------------------------------------------------ validation
def test_bad_arguments_are_einval_and_launch_nothing(torch_mod, codecs):
    torch = torch_mod
    import ctypes as C
    from llicti_amd import _lib
    from llicti_amd.codec import _ptr, _stream_ptr, mode_of_name
    c = codecs(5)
    H, W = 64, 96
    rgb = make_image("noise", H, W, 2)
    mode = mode_of_name("xrans2")
    cont, seg = c.encode(_dev(torch, rgb[None]), mode=mode)
    c.check()
    pix = _dev(torch, interleave(rgb, "rgba").reshape(-1))
    out = torch.full((H * W * 4,), POISON, dtype=torch.uint8, device="cuda:0")
    ws = c.workspace_v([H], [W], mode)
    Hs, Ws, modes = np.array([H], np.int32), np.array([W], np.int32), np.array([mode], np.int32)
    cont2, seg2 = torch.empty_like(cont), torch.empty_like(seg)
    before = {k: c.counter(k) for k in ("plan_builds", "plan_hits")}

    def enc(fmt, pitch, Hs_=Hs, modes_=modes):
        return c.L.llicti_encode_images_px(c.ctx, _ptr(pix), fmt, None, _ptr(pitch), 1, _ptr(Hs_), _ptr(Ws), _ptr(modes_), _ptr(ws), ws.numel(),
                                           _ptr(cont2), cont2.shape[1], _ptr(seg2), _stream_ptr(c.device))

    def dec(fmt, pitch, Hs_=Hs, modes_=modes, reduce=0):
        return c.L.llicti_decode_images_px(c.ctx, _ptr(cont), cont.shape[1], _ptr(seg), 1, _ptr(Hs_), _ptr(Ws), _ptr(modes_), 1, reduce, _ptr(ws), ws.numel(),
                                           _ptr(out), fmt, None, _ptr(pitch), _stream_ptr(c.device))

    short3, short4 = np.array([W * 3 - 1], np.uint64), np.array([W * 4 - 1], np.uint64)
    for call in (enc, dec):
        assert call(0, short3) == _lib.EINVAL                      # pitch < W * bpp
        assert call(2, short4) == _lib.EINVAL
        assert call(2, np.array([W * 3], np.uint64)) == _lib.EINVAL    # (a pitch that fits RGB8 is short for RGBA8)
        for bad in (4, -1, 17):
            assert call(bad, None) == _lib.EINVAL                  # unknown format
        assert call(2, None, Hs_=None) == _lib.EINVAL              # a null array the call needs
        assert call(2, None, modes_=None) == _lib.EINVAL
    assert dec(2, np.array([W * 2 - 1], np.uint64), reduce=1) == _lib.EINVAL      # the reduced window: 48 pixels of 4 bytes
    assert dec(2, np.array([W * 2], np.uint64), reduce=1) == _lib.OK
    c.check()                                                      # nothing was launched by the refused calls: the status is clean ...
    after = {k: c.counter(k) for k in before}
    assert after["plan_builds"] == before["plan_builds"] + 1 and after["plan_hits"] == before["plan_hits"], (before, after)      # ... and no plan was touched
    host = out.cpu().numpy().reshape(-1)
    assert (host[32 * W * 2:] == POISON).all() and np.array_equal(host[:32 * W * 2].reshape(32, 48, 4), interleave(rgb[:, ::2, ::2], "rgba", 255))
    assert _lib.lib().llicti_pixel_bytes(4) == 0 and _lib.lib().llicti_pixel_span(0, H, W, W * 3 - 1) == 0


# ------------------------------------------------------------------------------------------------ warm context
def test_warm_context_neither_syncs_nor_allocates(torch_mod, codecs):
    """More plans than the cache holds go through the new calls (their table blocks end up in the pool), then new sizes, pitches and formats:
    plan builds and nothing else -- no device synchronisation, no allocation."""
    torch = torch_mod
    from llicti_amd.codec import mode_of_name
    c = _new_codec(5)
    try:
        mode = mode_of_name("xrans2")

        def roundtrip(k, fmt):
            h, w = 32 + k, 40 + (3 * k) % 23
            bpp = _bpp(fmt)
            rgb = make_image("noise", h, w, k)
            pitch = w * bpp + k % 7
            buf = place([(interleave(rgb, fmt), 5, pitch, (h, w, bpp))])
            cont, seg = c.encode_px(_dev(torch, buf), [h], [w], mode, fmt, px_off=[5], pitch=[pitch])
            out = c.decode_px(cont, seg, [h], [w], mode, fmt, reduce=k % 2, px_off=[1], pitch=[pitch])
            return rgb, out, pitch

        for k in range(48):
            roundtrip(k, FORMATS[k % 4])
        c.check()
        before = {k: c.counter(k) for k in ("device_syncs", "device_allocs", "plan_builds", "block_waits")}
        for k in range(48, 60):
            rgb, out, pitch = roundtrip(k, FORMATS[(k + 1) % 4])
        c.check()
        after = {k: c.counter(k) for k in before}
        assert after["plan_builds"] == before["plan_builds"] + 24, (before, after)      # an encode and a decode plan (other offset / reduce) per size
        assert after["device_syncs"] == before["device_syncs"] and after["device_allocs"] == before["device_allocs"], (before, after)
        h, w = rgb.shape[1:]
        fmt = FORMATS[(59 + 1) % 4]
        s = 1 << (59 % 2)
        hr, wr = -(-h // s), -(-w // s)
        assert np.array_equal(read_window(out.cpu().numpy(), 1, pitch, hr, wr, _bpp(fmt)), interleave(rgb[:, ::s, ::s], fmt, 255))
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ Python level
def _model(torch, container):
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    torch.manual_seed(1337)
    return LLICTI(default_config(container=container)).to("cuda:0").eval()


@pytest.mark.parametrize("container", ["ac", "auto"])
def test_model_batches_in_hwc(torch_mod, container):
    """encode_batch_async(pixels=...) on [H, W, C] arrays gives the bytestream_lists of the planar list call; decode_batch_async(pixels=...)
    returns the [H, W, C] originals (alpha 255)."""
    torch = torch_mod
    m = _model(torch, container)
    sizes = [(67, 93), (67, 93)] if container == "ac" else [(150, 131), (96, 160)]      # (two sizes "auto" codes with one lane kind)
    rgbs = [make_image("smooth", h, w, 60 + i) for i, (h, w) in enumerate(sizes)]
    want = m.encode_batch_async(rgbs).lists()
    for fmt in FORMATS:
        hwc = [interleave(r, fmt) for r in rgbs]
        enc = m.encode_batch_async(hwc, pixels=fmt)
        assert enc.lists() == want, fmt
        assert (enc.Hs, enc.Ws) == ([h for h, _ in sizes], [w for _, w in sizes])
        m.codec().poison_workspace()
        outs = m.decode_batch_async(want, torch.device("cuda:0"), pixels=fmt)
        m.codec().check()
        assert isinstance(outs, list) and len(outs) == 2
        for o, r in zip(outs, rgbs):
            assert o.dtype == torch.uint8 and np.array_equal(o.cpu().numpy(), interleave(r, fmt, 255)), fmt
    flat, Hs, Ws = m.decode_batch_async(want, torch.device("cuda:0"), pixels="rgb", flat=True, reduce=1)
    m.codec().check()
    assert flat.numel() == 3 * sum(h * w for h, w in zip(Hs, Ws))
    assert np.array_equal(flat.cpu().numpy()[:3 * Hs[0] * Ws[0]].reshape(Hs[0], Ws[0], 3), interleave(rgbs[0][:, ::2, ::2], "rgb"))
    with pytest.raises(ValueError):
        m.encode_batch_async([interleave(rgbs[0], "rgb")], pixels="rgba")


@pytest.mark.parametrize("container", ["ac", "auto"])
def test_cli_roundtrip_equals_planar_model_call(torch_mod, tmp_path, container, capsys):
    """cli encode of a PPM writes the .llic bytes of the planar model call on the same image; cli decode writes the file the planar decode gives."""
    torch = torch_mod
    from llicti_amd import cli, fileio
    rgb = make_image("smooth", 67, 93, 21)
    src, mid, dst, ref = (str(tmp_path / n) for n in ("x.ppm", "x.llic", "y.ppm", "ref.ppm"))
    fileio.write_image(src, rgb)
    m = _model(torch, container)
    x = _dev(torch, rgb.astype(np.float32) / np.float32(255))[None]
    bl, _ = m.compress(x)
    assert cli.main(["encode", src, mid, "--container", container]) == 0
    n = sum(len(s) for r in bl for s in r)
    assert f"{src} -> {mid}: 93x67, {n} bytes, {8.0 * n / (67 * 93):.4f} bpp, " in capsys.readouterr().out
    assert open(mid, "rb").read() == fileio.dumps_llic(bl)
    assert cli.main(["decode", mid, dst]) == 0
    assert f"{mid} -> {dst}: 93x67, " in capsys.readouterr().out
    fileio.write_image(ref, (m.decompres(bl, torch.device("cuda:0"))[0] * 255).round().to(torch.uint8).cpu().numpy())
    assert open(dst, "rb").read() == open(ref, "rb").read()
    assert np.array_equal(fileio.read_image(dst), rgb)


def test_agent_directory_loader_codes_interleaved(torch_mod, tmp_path, caplog):
    """eval_model over a directory of image files (the interleaved path end to end) gives what it gives for the same images handed over in
    memory (the planar path): the same bytestream_lists and rates, every image lossless, the same per-image log lines but for the times."""
    import logging
    import re
    from llicti_amd import fileio
    from llicti_amd.agents.llicti_agent import LLICTIAgent
    from llicti_amd.config import default_config
    caplog.set_level(logging.INFO)
    rgbs = [make_image("smooth", h, w, 80 + i) for i, (h, w) in enumerate([(67, 93), (64, 96), (67, 93)])]
    for i, r in enumerate(rgbs):
        fileio.write_image(str(tmp_path / f"img_{i:02d}.ppm"), r)

    def run(test_data):
        caplog.clear()
        res = LLICTIAgent(default_config(test_data=test_data, eval_batch=2, container="auto", keep_streams=True)).run()
        lines = [r.message for r in caplog.records if "Check: Decoded img matches original" in r.message]
        return res, [re.match(r"\s*(\d+)\s+(\d+)x\s*(\d+) ", ln).groups() for ln in lines]
    res_f, heads_f = run(str(tmp_path))
    res_m, heads_m = run(rgbs)
    assert len(res_f) == len(res_m) == 3 and heads_f == heads_m and len(heads_f) == 3
    for rf, rm in zip(res_f, res_m):
        assert rf["bytestream_list"] == rm["bytestream_list"] and rf["rates"] == rm["rates"] and rf["bpsp"] == rm["bpsp"]
        assert rf["max_abs_err"] == 0.0 and rm["max_abs_err"] == 0.0
