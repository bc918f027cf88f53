"""tests/ref_rans.py -- the second, literal reading of the rANS containers -- applied to what the HIP kernels themselves wrote, with no oracle in
between: HipCodec.encode / encode_v / transcode -> ref_rans decode == input, with every check of the format text and every re-derivation of an
encoder choice on, the CDF rows taken from the HIP band CNN and table kernels; and corrupted containers put to the HIP decoders (on a poisoned
workspace) and to ref_rans: they refuse the same ones.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import ref_rans as rr
from conftest import load_state_dict
from helpers import B_VECTORS, RANS_TEST_IMAGES as IMAGES, corruptions, make_image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def codecs(torch_mod):
    """HipCodec per weight set: "trainedlike" / "rand1337" (config A), "b_rand1337" (config B), "cheap-single" (test_oracle_golden._cheap_case)."""
    from llicti_amd.codec import HipCodec
    cache = {}

    def get(wname, sd=None):
        if wname not in cache:
            c = HipCodec("cuda:0")
            if wname.startswith("b_"):
                c.set_model(60, 2)
            c.load_state_dict(sd if sd is not None else load_state_dict(wname))
            cache[wname] = c
        return cache[wname]
    yield get
    for c in cache.values():
        c.close()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class HipPlanes(rr.Planes):
    """CDF rows from the HIP kernels: the band CNN on the planes decoded so far (llicti_band_params_f32) and the table kernel (llicti_cdf_u16)."""

    def __init__(self, segs, codec, torch):
        super().__init__(segs)
        self.c, self.torch = codec, torch
        self._par = (None, None)

    def table(self, lvl, band, clr, R, C, minv, maxv):
        torch = self.torch
        planes = _dev(torch, self.planes[None])
        if self._par[0] != (lvl, band):
            fpl = _dev(torch, (self.planes.astype(np.float32) / np.float32(255))[None])
            self._par = ((lvl, band), self.c.band_params(fpl, lvl, band))
        mm = _dev(torch, np.array([[self.mm[1], self.mm[2], self.mm[4], self.mm[5]]], np.int32))
        tab = self.c.cdf_tables(planes, self._par[1], mm, lvl, band, clr)[0].cpu().numpy().view(np.uint16)
        assert tab.shape[0] == len(R) * len(C)
        return np.ascontiguousarray(tab[:, :maxv - minv + 2])


def _segs(cont_row, seg_row):
    from llicti_amd.codec import container_to_bytestream_list
    return rr.segments(container_to_bytestream_list(cont_row.cpu().numpy(), seg_row.cpu().numpy()))


def _ref_decode(torch, c, cont_row, seg_row, canonical=True):
    """ref_rans on one image's container, rows from the HIP kernels -> (uint8 [3, H, W], info)"""
    segs = _segs(cont_row, seg_row)
    planes, info = rr.decode_image(segs, HipPlanes(segs, c, torch), canonical=canonical)
    return c.unlift(_dev(torch, planes[None]))[0].cpu().numpy(), info


def _stream_classes(info):
    out = set()
    for f in info["streams"]:
        T, share = f["T"], f["share"]
        out |= {"empty-stream"} if share == 0 else set()
        if T:
            out.add("v4-one-chain" if f["one_chain"] else "v4-two-chains")
            out |= {"A=2-two-chains"} if (f["A"] == 2 and not f["one_chain"]) else set()
            out.add("T=whole-share" if T == share else "T<share")
            out |= {"T>=4096"} if T >= 4096 else set()
        out |= {"spill>0"} if f["spill"] else set()
        out |= {"field-255"} if (f["field"] == 255 and T == 8160) else set()
    return out


# (image of test_ref_rans.IMAGES or the cheap case, weights, xwide streams) -> classes the HIP ENCODER's own bytes must show
HIP_CASES = {
    "xrans1-smooth67": ("smooth67", "trainedlike", 1, {"v4-one-chain", "spill>0", "T<share"}),
    "xrans3-noise67": ("noise67", "rand1337", 3, {"v4-two-chains", "T=whole-share"}),
    "xrans1-noise67": ("noise67", "rand1337", 1, {"v4-two-chains", "spill>0", "T<share"}),
    "xrans5-noise32": ("noise32", "rand1337", 5, {"empty-stream"}),
    "xrans2-two64": ("two64", "trainedlike", 2, {"A=2-two-chains"}),
    "xrans1-flat192": ("flat192", "trainedlike", 1, {"field-255", "v4-one-chain", "T>=4096"}),
    "xrans4-cheap-single": ("cheap-single", None, 4, {"v4-one-chain", "T>=4096"}),
}


@pytest.mark.parametrize("name", list(HIP_CASES))
def test_hip_encoder_bytes_read_by_the_second_reader(torch_mod, codecs, name):
    """What the HIP encoder wrote, read by ref_rans with all checks and re-derivations on and the tables of the HIP kernels: the input, and the
    stream classes the case is there for."""
    from llicti_amd.codec import MODE_RANS
    torch = torch_mod
    iname, wname, M, classes = HIP_CASES[name]
    if iname == "cheap-single":
        from test_oracle_golden import _cheap_case
        sd, _, img = _cheap_case("single")
        c = codecs("cheap-single", sd)
    else:
        img, c = IMAGES[iname](), codecs(wname)
    cont, seg = c.encode(_dev(torch, img[None]), mode=MODE_RANS(M, wide=2))
    c.check()
    got, info = _ref_decode(torch, c, cont[0], seg[0])
    assert np.array_equal(got, img)
    assert info["header"]["M"] == M and classes <= _stream_classes(info), (name, _stream_classes(info))


def test_hip_encode_v_mixed_sizes_and_counts(torch_mod, codecs):
    """One llicti_encode_images_vm call, three sizes, a stream count per image: each container read by ref_rans."""
    from llicti_amd.codec import MODE_RANS
    torch = torch_mod
    c = codecs("trainedlike")
    imgs = [IMAGES["smooth67"](), IMAGES["noise33"](), IMAGES["two64"]()]
    Hs, Ws = [i.shape[1] for i in imgs], [i.shape[2] for i in imgs]
    modes = [MODE_RANS(1, wide=2), MODE_RANS(3, wide=2), MODE_RANS(2, wide=2)]
    flat = _dev(torch, np.concatenate([i.reshape(-1) for i in imgs]))
    cont, seg = c.encode_v(flat, Hs, Ws, modes)
    c.check()
    for b, img in enumerate(imgs):
        got, info = _ref_decode(torch, c, cont[b], seg[b])
        assert np.array_equal(got, img), b
        assert info["header"]["M"] == modes[b] & 0xFF


@pytest.mark.parametrize("iname,wname,Mlo", [("noise67", "rand1337", 1), ("smooth67", "trainedlike", 2)])
def test_hip_auto_count_is_the_rule(torch_mod, codecs, iname, wname, Mlo):
    """`auto`: the count in the header the DEVICE wrote is what the rule of include/llicti_hip.h gives, computed in plain Python from the
    last stage's frequencies as ref_rans decoded them; expensive symbols get a third more streams, a last stage that cannot fill two payloads one."""
    from llicti_amd.codec import MODE_RANS_AUTO
    torch = torch_mod
    c = codecs(wname)
    img = IMAGES[iname]()
    cont, seg = c.encode(_dev(torch, img[None]), mode=MODE_RANS_AUTO(Mlo))
    c.check()
    got, info = _ref_decode(torch, c, cont[0], seg[0])
    assert np.array_equal(got, img)
    assert info["header"]["M"] == rr.auto_pick(Mlo, info["last_freqs"]) == {"noise67": 2, "smooth67": 1}[iname]


@pytest.mark.parametrize("key", list(B_VECTORS))
def test_hip_config_b_container(torch_mod, codecs, key):
    """Config B (2 levels, byte 0 = 0xE9, 22 segments), an odd and an even shape: what the HIP encoder writes today is the frozen container that the CPU
    module reads (tests/golden/rans_b_vectors.npz), and ref_rans reads it with the tables of the HIP kernels too."""
    import os
    from conftest import GOLDEN
    from llicti_amd.codec import MODE_RANS
    torch = torch_mod
    kind, H, W, seed, wname, M = B_VECTORS[key]
    c = codecs("b_" + wname)
    img = make_image(kind, H, W, seed)
    cont, seg = c.encode(_dev(torch, img[None]), mode=MODE_RANS(M, wide=2))
    c.check()
    vec = np.load(os.path.join(GOLDEN, "rans_b_vectors.npz"))
    seg_h = seg[0].cpu().numpy()
    assert list(seg_h[:22]) == list(vec[f"{key}_seglen"]) and (seg_h[22:] == 0).all()
    assert cont[0, :int(seg_h.sum())].cpu().numpy().tobytes() == vec[f"{key}_bytes"].tobytes()
    assert len(_segs(cont[0], seg[0])) == 22
    got, info = _ref_decode(torch, c, cont[0], seg[0])
    assert np.array_equal(got, img), key
    assert info["header"]["nlevels"] == 2 and info["header"]["M"] == M


def test_hip_transcode_into_xrans(torch_mod, codecs):
    """64-lane containers transcoded on the device into xwide v4 ones: the target's bytes read by ref_rans."""
    from llicti_amd.codec import MODE_RANS
    torch = torch_mod
    c = codecs("rand1337")
    img = IMAGES["noise67"]()
    H, W = img.shape[1:]
    cont, seg = c.encode(_dev(torch, img[None]), mode=MODE_RANS(2))
    c.check()
    out, seg_out = c.transcode(cont, seg, [H], [W], MODE_RANS(2), MODE_RANS(3, wide=2))
    c.check()
    got, info = _ref_decode(torch, c, out[0], seg_out[0])
    assert np.array_equal(got, img)
    assert info["header"]["L"] == 256 and info["header"]["M"] == 3


# two per lane kind (a state bit, a main-region bit), a v3 stream's pad bits, then the xwide header field and the spill
HIP_CORRUPT = [("noise32", "rand1337", 0, 2, ("state", "main", "pad")), ("smooth32", "trainedlike", 1, 2, ("state", "main", "pad")),
               ("noise32", "rand1337", 2, 1, ("state", "main")), ("smooth67", "trainedlike", 2, 1, "field+spill"),
               ("b_noise33x40", "b_rand1337", 2, 3, ("state", "main", "top"))]          # config B (0xE9): the CPU module's corruption base


@pytest.mark.parametrize("iname,wname,wide,M,kinds", HIP_CORRUPT)
def test_hip_decoders_and_second_reader_refuse_the_same(torch_mod, codecs, iname, wname, wide, M, kinds):
    """Fifteen of the CPU module's single-bit corruptions, decoded by the HIP decoders next to an untouched neighbour on a poisoned workspace:
    image_status != 0 if and only if ref_rans refuses, equal pixels where both accept, the neighbour intact."""
    from llicti_amd._lib import EFORMAT, LlictiError
    from llicti_amd.codec import MODE_RANS, container_to_bytestream_list
    torch = torch_mod
    c = codecs(wname)
    img = IMAGES[iname]()
    H, W = img.shape[1:]
    mode = MODE_RANS(M, wide=wide)
    cont, seg = c.encode(_dev(torch, np.stack([img, img])), mode=mode)
    c.check()
    seg_h = seg.cpu().numpy()
    bl = container_to_bytestream_list(cont[1].cpu().numpy(), seg_h[1])
    L = 64 << wide
    flips = corruptions(bl[1][0], L, "v4" if wide == 2 else "v3", seed=11)
    if kinds == "field+spill":
        from helpers import xwide_stream_header
        field, one_chain, main_bits = xwide_stream_header(bl[1][0])
        assert one_chain == 1 and field == 47                   # T = 1504 of 1551, 74 bits of spill under the main region
        picked = [("field", main_bits), ("one-chain flag", main_bits + 8), ("spill", 0), ("spill", 40)]
    else:
        picked = [[f for f in flips if f[0] == kind][0] for kind in kinds if kind != "pad"]     # the first flip of its kind in the CPU module's fixed order
        if "pad" in kinds:
            # the highest of the unused bits on top of a v3 bit region's last byte: both decoders ignored them until ref_rans read the text
            assert (bl[1][0][1] >> 3) & 7 > 0
            picked.append(("pad", [f for f in flips if f[0] == "top"][-1][1]))
    off = int(seg_h[1, :4].sum())
    for kind, bit in picked:
        bad = cont.clone()
        bad[1, off + (bit >> 3)] ^= 1 << (bit & 7)
        c.workspace(2, H, W, mode)
        c.poison_workspace(0xA5)
        rec = c.decode(bad, seg, H, W, mode=mode)
        try:
            c.check()
        except LlictiError as e:
            assert e.code == EFORMAT, (kind, bit, e)          # a malformed container and nothing else: anything else ends the test here
        status = list(c.image_status(2))
        assert status[0] == 0 and np.array_equal(rec[0].cpu().numpy(), img), (kind, bit)         # the untouched neighbour
        try:
            got, _ = _ref_decode(torch, c, bad[1], seg[1], canonical=False)
        except rr.Refused:
            got = None
        assert (status[1] != 0) == (got is None), (kind, bit, status, "ref_rans " + ("refuses" if got is None else "accepts"))
        if got is not None:
            assert np.array_equal(rec[1].cpu().numpy(), got), (kind, bit)
