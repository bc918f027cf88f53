"""All seven decoder paths on adversarial mixtures (run with -m gpu on an MI355X).  The mixture CDF entry is evaluated in nine places of the kernels
(two on the encoder's side, seven on the decoders' -- nine callers of one statement, numerics.hpp's mix_term / entry_from_sum); the encoder's two are held to the oracle at hand-made parameter rows
(test_hip_parity.py::test_cdf_*_kernel_adversarial_params), the decoders take theirs from the CNN inside the decode calls.  Here a model
whose last layer emits chosen biases (tests/mixture_regimes.py) hands every decoder the same regimes from the INPUTS: nothing in the library
is switched, forced or observed.  Per regime: four 67 x 93 images as one batch through the reference format with full tables and with
anchors, rans4, wrans3, xrans1, xrans3 and the "auto" encoder mode (the size rule's count, decoded by each header's mode) -- encode, check(),
decode on a poisoned workspace, check(), pixels equal the originals, every image's status clean -- and the containers of images (a) and (b)
equal the oracle's byte for byte.  Which symbol classes those images hold is asserted on the CPU (tests/test_mixture_regimes_cpu.py).
Wall time on one MI355X: 0.2 - 0.5 s per regime, 0.02 s per config-B twin."""
import numpy as np
import pytest

import mixture_regimes as mr

pytestmark = pytest.mark.gpu

H, W = mr.H, mr.W
# (path, container name, ac_anchor_min_batch during the decode, kind of the oracle's container it must equal)
PATHS = (("ac_tables", "ac", 96, "ac"), ("ac_anchors", "ac", 1, "ac"), ("rans4", "rans4", 96, "rans4"), ("wrans3", "wrans3", 96, "wrans3"),
         ("xrans1", "xrans1", 96, "xrans1"), ("xrans3", "xrans3", 96, "xrans3"), ("xauto", None, 96, "xauto"))


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _auto_count(nlevels=5):
    """the size rule's stream count, at least one: 67 x 93 is below the rule's smallest xwide image"""
    from llicti_amd.codec import image_streams
    return max(1, image_streams(H, W, nlevels))


_oracle = {}


def _oracle_side(name):
    """images, and the oracle's containers of images (a) and (b) per kind: once per regime and process (their round trips through the oracle
    are tests/test_mixture_regimes_cpu.py's)"""
    from oracle import oracle as orc
    if name not in _oracle:
        imgs = mr.regime_images(name)
        W_o = mr.oracle_weights(name)
        want = {}
        for kind in ("ac", "rans4", "wrans3", "xrans1", "xrans3"):
            want[kind] = [orc.encode_image(imgs[b], W_o) if kind == "ac" else orc.encode_image_rans(imgs[b], W_o, *mr.RANS_KINDS[kind]) for b in (0, 1)]
        want["xauto"] = [orc.encode_image_rans(imgs[b], W_o, _auto_count(), 2, auto=True) for b in (0, 1)]     # (the same rule in the oracle)
        _oracle[name] = (imgs, W_o, want)
    return _oracle[name]


def _pinned_rows_arrive(torch, c, x, name, W_o=None):
    """band_params at level 0, band x10 returns the pinned biases bit for bit in the pinned channels (and, where the oracle has the model, its
    own 60 outputs bit for bit): the row reached the coder"""
    from oracle import oracle as orc
    planes, fplanes, _ = c.lift(x)
    p60 = c.params60(c.band_params(fplanes, 0, 2)).cpu().numpy()
    pins = mr.pinned(name)
    assert pins
    for ch, want in pins.items():
        assert (p60[..., ch].view(np.uint32) == np.float32(want).view(np.uint32)).all(), (name, ch, want)
    if W_o is not None:
        ref = orc.band_params(planes[1].cpu().numpy(), 0, 2, W_o)
        assert np.array_equal(p60[1].view(np.uint32), ref.view(np.uint32)), name


def _decode_poisoned(c, cont, seg, modes):
    """decode on a workspace that holds no trace of the encode (test_hip_parity._decode_poisoned's method); `modes`: the containers' own,
    one per image -- one call where they agree, the per-image call where an "auto" encode picked different counts"""
    B = cont.shape[0]
    if len(set(modes)) == 1:
        c.workspace(B, H, W, modes[0])
        c.poison_workspace(0xA5)
        out = c.decode(cont, seg, H, W, mode=modes[0])
    else:
        c.workspace_v([H] * B, [W] * B, modes)
        c.poison_workspace(0xA5)
        out = c.decode_v(cont, seg, [H] * B, [W] * B, modes).view(B, 3, H, W)
    c.check()
    return out


def _run_paths(torch, c, x, paths, name, want, nlevels=5):
    from llicti_amd.codec import MODE_RANS_AUTO, container_to_bytestream_list, mode_of_name
    B = x.shape[0]
    rgb = x.cpu().numpy()
    for path, cname, anchors, kind in paths:
        mode = MODE_RANS_AUTO(_auto_count(nlevels)) if cname is None else mode_of_name(cname)      # "auto": the encoder picks each image's count
        cont, seg = c.encode(x, mode=mode)
        c.check()
        modes = c.container_modes(cont)
        if cname is not None:
            assert modes == [mode] * B, (name, path, modes)
        if kind is not None and want is not None:
            cont_h, seg_h = cont.cpu().numpy(), seg.cpu().numpy()
            for b in (0, 1):
                assert container_to_bytestream_list(cont_h[b], seg_h[b]) == want[kind][b], (name, path, "image " + "ab"[b])
        c.set_tuning("ac_anchor_min_batch", anchors)
        try:
            rec = _decode_poisoned(c, cont, seg, modes)
        finally:
            c.set_tuning("ac_anchor_min_batch", 96)
        got = rec.cpu().numpy()
        for b in range(B):
            assert np.array_equal(got[b], rgb[b]), (name, path, "image " + "abcd"[b], int((got[b] != rgb[b]).sum()))
        assert not c.image_status(B).any(), (name, path)


@pytest.mark.parametrize("name", mr.REGIME_NAMES)
def test_every_decoder_path_on_regime(torch_mod, name):
    from llicti_amd.codec import HipCodec
    torch = torch_mod
    imgs, W_o, want = _oracle_side(name)
    c = HipCodec("cuda:0")
    try:
        c.load_state_dict(mr.regime_state_dict(name))
        x = _dev(torch, np.stack(imgs))
        _pinned_rows_arrive(torch, c, x, name, W_o)
        _run_paths(torch, c, x, PATHS, name, want)
    finally:
        c.close()


@pytest.mark.parametrize("name", mr.B_NAMES)
def test_config_b_twin_on_regime(torch_mod, name):
    """The 60-wide, 2-level model under the same pinned rows: the reference format and xrans2, the formats config B has (no oracle of config B:
    lossless, clean and the rows arrived)."""
    from llicti_amd.codec import HipCodec
    torch = torch_mod
    c = HipCodec("cuda:0")
    try:
        c.set_model(60, 2)
        c.load_state_dict(mr.regime_state_dict(name))
        x = _dev(torch, np.stack(mr.regime_images(name)))
        _pinned_rows_arrive(torch, c, x, name)
        _run_paths(torch, c, x, (("ac_tables", "ac", 96, None), ("ac_anchors", "ac", 1, None), ("xrans2", "xrans2", 96, None)), name, None, nlevels=2)
    finally:
        c.close()
