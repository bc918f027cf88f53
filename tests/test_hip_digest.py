"""Pixel digests on the GPU (run with -m gpu on an MI355X): llicti_crc32_planes at every seam of its kernel, llicti_digest_images behind every
whole-batch encode and decode form, detection of a damaged stream, the calling contract, the caller's stream, and the model / archive / command
line layers.  EVERY REFERENCE IS zlib.crc32 OF THE SOURCE PIXELS as planar uint8 [3][H][W] bytes -- never the library, never a decode."""
import os
import zlib

import numpy as np
import pytest

from conftest import load_state_dict
from helpers import StreamGate, make_image

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MIXED = [(67, 93), (32, 32), (93, 67), (64, 48)]            # the suite's mixed-size batch
GATE_MS = 100.0


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
            c = cache[nlev] = HipCodec(DEV)
            if nlev == 2:
                c.set_model(60, 2)
            c.load_state_dict(load_state_dict("b_trainedlike" if nlev == 2 else "trainedlike"))
        return cache[nlev]
    yield get
    for c in cache.values():
        c.close()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _crc(rgb):
    return zlib.crc32(np.ascontiguousarray(rgb).tobytes()) & 0xFFFFFFFF


def _lift_np(rgb):
    """uint8 [.., 3, H, W] -> int16 planes (Y - 127, Co, Cg): the integer YCoCg-R lift, in numpy"""
    R, G, B = (rgb[..., k, :, :].astype(np.int32) for k in range(3))
    Co = R - B
    t = B + (Co >> 1)
    Cg = G - t
    return np.stack((t + (Cg >> 1) - 127, Co, Cg), axis=-3).astype(np.int16)


# ------------------------------------------------------------------------------------------------ 1. the kernel at its seams
def _seam_counts():
    from llicti_amd.codec import crc32_geometry
    L, G = crc32_geometry()
    return [1, 2, 3, 5, L - 1, L, L + 1, 2 * L + 1, G - 1, G, G + 1, 2 * G + L + 3]


def _shapes_of(n):
    """1 x n where that is a legal width; else 2 x ceil(n / 2) and 3 x k on either side of n / 3 -- odd plane bases, planes that are no multiple
    of 4 or 8 --, and H x W = n exactly where n has such a factor pair"""
    if n <= 8160:
        return [(1, n)]
    out = [(h, w) for h, w in [(2, -(-n // 2)), (3, -(-n // 3)), (3, n // 3)] if w <= 8160]      # (2G + L + 3 is too wide for two rows)
    exact = next(((h, n // h) for h in range(2, 64) if n % h == 0 and n // h <= 8160), None)
    assert out
    return sorted(set(out + ([exact] if exact else [])))


@pytest.mark.parametrize("k", range(12))
def test_crc32_planes_at_every_seam(torch_mod, codecs, k):
    torch, c = torch_mod, codecs()
    n = _seam_counts()[k]
    for H, W in _shapes_of(n):
        rgb = np.random.default_rng(1000 * k + H).integers(0, 256, (3, 3, H, W), dtype=np.uint8)      # three distinct images per call
        got = c.crc32_planes(_dev(torch, _lift_np(rgb)))
        assert got.dtype == torch.int64 and got.tolist() == [_crc(rgb[b]) for b in range(3)], (n, H, W)


@pytest.mark.parametrize("H,W", [(67, 93), (32, 32)])
def test_crc32_planes_on_lift(torch_mod, codecs, H, W):
    torch, c = torch_mod, codecs()
    rgb = np.stack([make_image(("smooth", "noise", "noise")[b], H, W, 70 + b) for b in range(3)])
    planes = c.lift(_dev(torch, rgb))[0]
    assert np.array_equal(planes.cpu().numpy(), _lift_np(rgb))
    assert c.crc32_planes(planes).tolist() == [_crc(rgb[b]) for b in range(3)]


def test_crc32_planes_all_zero_and_all_255(torch_mod, codecs):
    torch, c = torch_mod, codecs()
    rgb = np.stack([np.zeros((3, 67, 93), np.uint8), np.full((3, 67, 93), 255, np.uint8), make_image("noise", 67, 93, 9)])
    assert c.crc32_planes(c.lift(_dev(torch, rgb))[0]).tolist() == [_crc(rgb[b]) for b in range(3)]
    assert len({_crc(rgb[b]) for b in range(3)}) == 3


def test_crc32_planes_largest_image_offsets_past_2_31_and_slices(torch_mod, codecs):
    """Nine images of 8160 x 8160 in one call: 8,129 groups per image (the fold kernel walks them 256 at a time), byte offsets past 2^31 from
    the sixth image on, and more groups than the partials scratch holds at once, so the images go in two slices.  Eight images are black --
    one zlib pass over 200 MB of zeros serves them all -- and the ninth, behind them, is random; everything is made on the device."""
    torch, c = torch_mod, codecs()
    H = W = 8160
    B = 9
    planes = torch.zeros((B, 3, H, W), dtype=torch.int16, device=DEV)
    planes[:, 0] = -127                                            # black: Y - 127 = -127, Co = Cg = 0
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    rgb = torch.randint(0, 256, (3, H, W), dtype=torch.int32, device=DEV, generator=g)
    Co = rgb[0] - rgb[2]
    t = rgb[2] + (Co >> 1)
    Cg = rgb[1] - t
    planes[B - 1] = torch.stack((t + (Cg >> 1) - 127, Co, Cg)).to(torch.int16)
    got = c.crc32_planes(planes).tolist()
    black = zlib.crc32(bytes(3 * H * W)) & 0xFFFFFFFF
    assert got[:B - 1] == [black] * (B - 1)
    assert got[B - 1] == _crc(rgb.to(torch.uint8).cpu().numpy())
    del planes


# ------------------------------------------------------------------------------------------------ 2. whole calls
CASES = {"auto": (5, "auto", MIXED), "rans4": (5, "rans4", MIXED), "ac": (5, "ac", [(32, 32)] * 4), "config_b": (2, "xrans2", MIXED)}


class Coded:
    """One batch, encoded once: the source pixels' CRCs (zlib), the containers, the modes of the encode and of a decode"""

    def __init__(self, torch, c, nlev, name, sizes, seed=300):
        from llicti_amd.codec import auto_modes, mode_of_name
        self.c, self.sizes = c, list(sizes)
        self.Hs, self.Ws = [h for h, _ in sizes], [w for _, w in sizes]
        self.rgbs = [make_image(("smooth", "noise")[i % 2], h, w, seed + i) for i, (h, w) in enumerate(sizes)]
        self.src = [_crc(r) for r in self.rgbs]
        self.enc_mode = auto_modes(self.sizes, nlev) if name == "auto" else mode_of_name(name)
        self.flat = _dev(torch, np.concatenate([r.reshape(-1) for r in self.rgbs]))
        self.cont, self.seg = c.encode_v(self.flat, self.Hs, self.Ws, self.enc_mode)
        self.enc_digests = c.digests(self.Hs, self.Ws, self.enc_mode)      # (directly behind the encode)
        c.check()
        self.mode = c.container_modes(self.cont)

    def digests_after(self, decode, reduce=None):
        """poison the workspace, run `decode`, digest what it left"""
        self.c.poison_workspace()
        decode()
        crc, have = self.c.digests(self.Hs, self.Ws, self.mode, reduce=reduce)
        return crc.tolist(), have.tolist()


@pytest.fixture(scope="module")
def coded(torch_mod, codecs):
    cache = {}

    def get(case):
        if case not in cache:
            nlev, name, sizes = CASES[case]
            cache[case] = Coded(torch_mod, codecs(nlev), nlev, name, sizes)
        return cache[case]
    return get


@pytest.mark.parametrize("case", list(CASES))
def test_digests_behind_the_encode(torch_mod, coded, case):
    k = coded(case)
    crc, have = k.enc_digests
    assert crc.dtype == torch_mod.int64 and crc.tolist() == k.src and have.tolist() == [1] * 4


@pytest.mark.parametrize("case", list(CASES))
def test_digests_do_not_depend_on_the_sink(torch_mod, coded, case):
    torch, k = torch_mod, coded(case)
    c, a = k.c, (k.cont, k.seg, k.Hs, k.Ws, k.mode)
    sinks = {
        "decode_v": lambda: c.decode_v(*a),
        "decode_px": lambda: c.decode_px(*a, "bgra"),
        "decode_tensor": lambda: c.decode_tensor(*a, (16, 16), dtype=torch.float16),
        "decode_tensor_resized": lambda: c.decode_tensor_resized(*a, (8, 8), None, antialias=False),
        "decode_tensor_views": lambda: c.decode_tensor_views(*a, [dict(size=(8, 8), antialias=False)]),
    }
    for name, fn in sinks.items():
        assert k.digests_after(fn) == (k.src, [1] * 4), name
        c.check()
    # the planar decode really returned the pixels (the yardstick of the yardstick)
    flat = c.decode_v(*a).cpu().numpy()
    assert np.array_equal(flat, np.concatenate([r.reshape(-1) for r in k.rgbs]))


@pytest.mark.parametrize("case", list(CASES))
def test_per_image_reduce(coded, case):
    """The reference format decodes at ONE reduce per call (differing values are LLICTI_EINVAL): its batch is decoded in full and only the
    digest call is given the values -- the images it is told were reduced get no digest and are not read."""
    k = coded(case)
    red = [0, 2, 0, 1]
    crc, have = k.digests_after(lambda: k.c.decode_v(k.cont, k.seg, k.Hs, k.Ws, k.mode, reduce=0 if case == "ac" else red), reduce=red)
    assert have == [1, 0, 1, 0] and crc == [k.src[0], 0, k.src[2], 0]


@pytest.mark.parametrize("case", list(CASES))
def test_scalar_reduce_has_no_digest(coded, case):
    k = coded(case)
    crc, have = k.digests_after(lambda: k.c.decode_v(k.cont, k.seg, k.Hs, k.Ws, k.mode, reduce=1), reduce=1)
    assert have == [0] * 4 and crc == [0] * 4


# ------------------------------------------------------------------------------------------------ 3. detection
def test_a_damaged_level0_stream_changes_the_digest(torch_mod, coded):
    """One byte of image 1's stream 0 is flipped where level 0's bits lie -- a stream's bit region is read downwards, coarse levels first, so
    its lower part belongs to level 0 (three quarters of the symbols).  The decode is the ordinary decode of a damaged container."""
    torch, k = torch_mod, coded("rans4")
    seg = k.seg.cpu().numpy()
    start, length = int(seg[1, :4].sum()), int(seg[1, 4])
    assert length > 2 + 248 + 64                                   # (T field, bit region, 64 x 31-bit states)
    pos = start + 2 + (length - 2 - 248) // 4
    bad = k.cont.clone()
    bad[1, pos] ^= 0x10
    k.c.poison_workspace()
    k.c.decode_v(bad, k.seg, k.Hs, k.Ws, k.mode)
    crc, have = k.c.digests(k.Hs, k.Ws, k.mode)
    status = k.c.image_status(4)
    crc = crc.tolist()
    assert crc[1] != k.src[1], status
    assert [crc[0], crc[2], crc[3]] == [k.src[0], k.src[2], k.src[3]] and have.tolist() == [1] * 4
    try:
        k.c.check()                                                # (clears the latched word, whatever it says)
    except Exception:
        pass


# ------------------------------------------------------------------------------------------------ 4. calling contract
def test_no_cached_plan_is_einval(coded):
    from llicti_amd import _lib
    k = coded("rans4")
    with pytest.raises(_lib.LlictiError) as e:
        k.c.digests([40, 44], [48, 52], k.mode[:2])
    assert e.value.code == _lib.EINVAL and "no plan is cached" in str(e.value)


def test_warm_digests_build_allocate_and_synchronise_nothing(coded):
    k = coded("rans4")
    k.c.decode_v(k.cont, k.seg, k.Hs, k.Ws, k.mode)
    names = ("plan_builds", "device_allocs", "device_syncs")
    before = [k.c.counter(n) for n in names]
    first = k.c.digests(k.Hs, k.Ws, k.mode)[0]
    second = k.c.digests(k.Hs, k.Ws, k.mode)[0]
    assert [k.c.counter(n) for n in names] == before
    assert first.tolist() == second.tolist() == k.src
    # the flags of a call with reduced images travel in a pooled block: warm, that allocates nothing either
    k.c.decode_v(k.cont, k.seg, k.Hs, k.Ws, k.mode, reduce=[0, 1, 0, 1])
    k.c.digests(k.Hs, k.Ws, k.mode, reduce=[0, 1, 0, 1])
    k.c.check()                                                    # (the pool's blocks are handed out again once their last user has finished)
    before = [k.c.counter(n) for n in names]
    assert k.c.digests(k.Hs, k.Ws, k.mode, reduce=[0, 1, 0, 1])[1].tolist() == [1, 0, 1, 0]
    assert [k.c.counter(n) for n in names] == before


# ------------------------------------------------------------------------------------------------ 5. the caller's stream
def test_encode_and_digests_on_a_gated_stream(torch_mod, coded):
    """encode + digests are enqueued on a non-blocking stream behind a gate while the input buffer still holds a DECOY; the real images are
    copied over it on that stream, in front of the calls.  Work not ordered behind the stream would see the decoy."""
    torch, k = torch_mod, coded("rans4")
    c = k.c
    decoy = _dev(torch, np.concatenate([make_image(("noise", "smooth")[i % 2], h, w, 900 + i).reshape(-1) for i, (h, w) in enumerate(k.sizes)]))
    s = torch.cuda.Stream(device=DEV)
    gate = StreamGate(torch, DEV)
    buf = decoy.clone()

    def enqueue():
        buf.copy_(k.flat, non_blocking=True)
        c.encode_v(buf, k.Hs, k.Ws, k.enc_mode)
        crc, have = c.digests(k.Hs, k.Ws, k.enc_mode)
        return crc.clone(), have.clone()
    with torch.cuda.stream(s):                                     # an ungated pass: kernels loaded, the stream's allocator pool warm
        enqueue()
    torch.cuda.synchronize()
    buf.copy_(decoy)
    torch.cuda.synchronize()
    _, end = gate.hold(s, GATE_MS)
    with torch.cuda.stream(s):
        crc, have = enqueue()
    assert end.query() is False, "the gate ran out before the last call was enqueued: the run proves nothing"
    s.synchronize()
    assert crc.tolist() == k.src and have.tolist() == [1] * 4
    c.check()


# ------------------------------------------------------------------------------------------------ 6. model, archive, command line
def _model(torch, container):
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    torch.manual_seed(1337)
    return LLICTI(default_config(container=container)).to(DEV).eval()


def test_model_layer(torch_mod, tmp_path):
    torch = torch_mod
    from llicti_amd import archive
    m = _model(torch, "xrans2")
    sizes = [(96, 160), (67, 93), (64, 64)]
    rgbs = [make_image(("smooth", "noise")[i % 2], h, w, 50 + i) for i, (h, w) in enumerate(sizes)]
    src = [_crc(r) for r in rgbs]
    enc = m.encode_batch_async(rgbs, digests=True)
    assert enc.digests() == src
    plain = m.encode_batch_async(rgbs)
    with pytest.raises(ValueError):
        plain.digests()
    # an archive batch decoded to a small tensor: the digests are the whole images'
    blob, rec_off = enc.records()
    path = str(tmp_path / "m.llia")
    with archive.ArchiveWriter(path, m.codec().nseg) as aw:
        aw.append_records(blob, rec_off, ["a", "b", "c"])
    with archive.ArchiveReader(path) as ar:
        order = [2, 0, 1]
        out = m.decode_batch_async(ar.read_batch(order), tensor=dict(size=(16, 16), dtype=torch.float16))
        crc, have = m.last_digests()
        assert tuple(out.shape) == (3, 3, 16, 16) and crc.tolist() == [src[i] for i in order] and have.tolist() == [1, 1, 1]
        want = torch.tensor([src[i] for i in order], dtype=torch.int64, device=DEV)
        assert not bool((crc != want).any())                       # (a loader's compare: one device `!=`)
        m.decode_batch_async(ar.read_batch(order), reduce=[0, 1, 0])
        crc, have = m.last_digests()
        assert have.tolist() == [1, 0, 1] and crc.tolist() == [src[2], 0, src[1]]
    m.codec().check()
    # progressive records pay a decode: its digests are held against the encode's
    enc2 = m.encode_batch_async(rgbs, digests=True)
    assert len(enc2.records(progressive=True)) == 3
    assert enc2.digests(verify=True) == src
    enc2._crc_decoded = [src[0], src[1] ^ 1, src[2]]
    with pytest.raises(ValueError, match=r"images \[1\]"):
        enc2.digests(verify=True)


def test_cli_pack_digests_info_verify(torch_mod, tmp_path, capsys):
    from llicti_amd import archive, cli, digest, fileio
    sizes = [(64, 96), (67, 93), (96, 64)]
    rgbs = [make_image(("smooth", "noise")[i % 2], h, w, 80 + i) for i, (h, w) in enumerate(sizes)]
    srcs = []
    for i, r in enumerate(rgbs):
        srcs.append(str(tmp_path / f"img_{i}.ppm"))
        fileio.write_image(srcs[-1], r)
    arc, bare = str(tmp_path / "set.llia"), str(tmp_path / "bare.llia")
    assert cli.main(["pack", arc] + srcs + ["--container", "xrans2", "--batch", "2", "--digests"]) == 0
    assert cli.main(["pack", bare] + srcs + ["--container", "xrans2", "--batch", "2"]) == 0
    assert open(arc, "rb").read() == open(bare, "rb").read()       # the archive's bytes do not know about the manifest
    assert os.path.exists(arc + ".lldg") and not os.path.exists(bare + ".lldg")
    with archive.ArchiveReader(arc) as ar:
        assert digest.read_manifest(arc + ".lldg", ar) == [_crc(r) for r in rgbs]
        off = [int(v) for v in ar.offsets]
    capsys.readouterr()
    assert cli.main(["info", arc]) == 0
    text = capsys.readouterr().out
    assert f"img_1: 93x67, container xrans2" in text and f"crc32 {_crc(rgbs[1]):08x}" in text
    assert cli.main(["info", bare]) == 0
    assert "crc32" not in capsys.readouterr().out
    assert cli.main(["verify", arc, "--batch", "2"]) == 0
    assert "3 of 3 images verified" in capsys.readouterr().out
    assert cli.main(["verify", bare]) == 2                         # (no manifest)
    capsys.readouterr()
    # one payload byte of image 1 flipped in the file
    data = bytearray(open(arc, "rb").read())
    data[(off[1] + off[2]) // 2] ^= 0x04
    with open(arc, "wb") as fh:
        fh.write(bytes(data))
    assert cli.main(["verify", arc]) == 1
    text = capsys.readouterr().out
    assert "img_1:" in text and "img_0:" not in text and "img_2:" not in text and "2 of 3 images verified, 1 differ" in text


def test_cli_encode_digest_and_decode_crc32(torch_mod, tmp_path, capsys):
    from llicti_amd import cli, fileio
    rgb = make_image("smooth", 67, 93, 33)
    src, llic, out = str(tmp_path / "x.ppm"), str(tmp_path / "x.llic"), str(tmp_path / "y.ppm")
    fileio.write_image(src, rgb)
    assert cli.main(["encode", src, llic, "--container", "xrans2", "--digest"]) == 0
    assert f"crc32={_crc(rgb):08x}" in capsys.readouterr().out
    assert cli.main(["decode", llic, out, "--crc32", f"{_crc(rgb):08x}"]) == 0
    assert np.array_equal(fileio.read_image(out), rgb)
    assert cli.main(["decode", llic, out, "--crc32", f"{_crc(rgb) ^ 1:08x}"]) == 1
    assert "DIFFERS" in capsys.readouterr().out
