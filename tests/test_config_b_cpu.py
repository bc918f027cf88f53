"""Config B (configs/llicti_B.json: 60-wide heads, 2 levels) on the host side: config check, the model's parameters, the weight pack and the
header functions of the C-ABI against their Python twins.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch


def _b_config(**over):
    from llicti_amd.config import CONFIG_B, default_config
    c = default_config(**CONFIG_B)
    c.update(over)
    return c


def _b_model(seed=1337):
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    torch.manual_seed(seed)
    return LLICTI(_b_config())


def test_config_b_accepted_and_other_shapes_refused():
    from llicti_amd.config import check_supported, default_config, model_shape
    check_supported(_b_config())
    assert model_shape(_b_config()) == (60, 2) and model_shape(default_config()) == (88, 5)
    for over in ({"dwtlevels": [0, 1, 2, 3, 4], "useprevlevNN": [False, True, True, True, True]},      # 60-wide heads, 5 levels
                 {"chs": [88, 1, 1, 1, 1]},                                                               # 88-wide heads, 2 levels
                 {"chs": [64, 1, 1, 1, 1]}, {"dwtlevels": [0, 1, 2]}, {"useprevlevNN": [False, False]}, {"num_mixtures": 3}):
        with pytest.raises(NotImplementedError):
            check_supported(_b_config(**over))


def test_config_b_state_dict_keys_and_shapes():
    from llicti_amd.weights import expected_keys
    sd = _b_model().state_dict()
    assert len(sd) == 33
    for k in expected_keys():
        assert k in sd, k
        v = sd[k]
        if ".layer0_" in k and k.endswith(".weight"):
            assert v.shape[:2] == (240, 3) and tuple(v.shape[2:]) in ((4, 4), (3, 4), (4, 3)), (k, v.shape)
        elif ".layer0_" in k:
            assert v.shape == (240,), (k, v.shape)
    p = "entropymodel.entmdls_scale_band.0.0."
    assert sd[p + "layers1toL.0.weight"].shape == (240, 60, 1, 1)
    assert sd[p + "layers1toL.2.weight"].shape == (60, 60, 1, 1)
    assert sd[p + "layers1toL.2.bias"].shape == (60,)


def test_config_b_pack_and_head_inference():
    from llicti_amd.weights import K0, head_of_state_dict, pack_state_dict
    sd = _b_model().state_dict()
    assert head_of_state_dict(sd) == 60
    pk = pack_state_dict(sd)
    for b in range(3):
        d, p = pk[b], f"entropymodel.entmdls_scale_band.0.{b}."
        assert d["head"] == 60 and d["K0"] == K0[b]
        assert d["w0"].shape == (240, K0[b]) and d["b0"].shape == (240,)
        assert d["w1"].shape == (240, 60) and d["w2"].shape == (60, 60) and d["b2"].shape == (60,)
        assert np.array_equal(d["w1"], sd[p + "layers1toL.0.weight"].numpy().reshape(240, 60))
        assert np.array_equal(d["w2"], sd[p + "layers1toL.2.weight"].numpy().reshape(60, 60))
    # the first conv of band 0 is 4x4: its flattening is (ci, ky, kx), the canonical K order
    w = sd["entropymodel.entmdls_scale_band.0.0.layer0_00_11.weight"].numpy()
    assert np.array_equal(pk[0]["w0"], w.reshape(240, 48))
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    assert head_of_state_dict(LLICTI(default_config()).state_dict()) == 88


def test_checkpoint_of_the_other_model_is_refused():
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    from llicti_amd.weights import load_reference_state_dict
    a, b = LLICTI(default_config()), _b_model()
    with pytest.raises(ValueError, match="60-wide"):
        load_reference_state_dict(a, b.state_dict())
    with pytest.raises(ValueError, match="88-wide"):
        load_reference_state_dict(b, a.state_dict())
    load_reference_state_dict(b, _b_model(7).state_dict())          # the same model loads


def _pad2(H, W):
    v = 0
    for lvl in range(2):
        Hl, Wl = -(-H // (1 << lvl)), -(-W // (1 << lvl))
        v = 4 * v + 2 * (Hl & 1) + (Wl & 1)
    return v


@pytest.mark.parametrize("H,W", [(32, 32), (67, 93), (512, 768), (764, 1020)])
def test_header_functions_on_config_b_headers(H, W):
    """llicti_header_dims / llicti_header_mode (host functions of the library) against codec.header_dims / mode_of_header on config B's headers:
    the reference format (byte 0 = 2 scales) and xwide v4 (0xE9, the count in the pad field), and the A-only readings of them refused."""
    from llicti_amd import _lib
    from llicti_amd.codec import MODE_AC, MODE_RANS, header_dims, levels_of_header, mode_of_header
    L = _lib.lib()
    h1, w1 = -(-(-(-H // 2)) // 2), -(-(-(-W // 2)) // 2)
    pad = _pad2(H, W)
    for b0, u, want in [(2, 0, MODE_AC)] + [(0xE9, u, MODE_RANS(u if u <= 32 else {33: 64, 34: 128}[u], wide=2)) for u in (1, 12, 18, 32, 33)]:
        hdr = bytes([b0, h1, w1]) + bytes(12) + int(pad | (u << 10)).to_bytes(2, "little")
        assert header_dims(hdr) == (H, W)
        m = C.c_int(-1)
        assert L.llicti_header_mode((C.c_uint8 * 17).from_buffer_copy(hdr), C.byref(m)) == 0
        assert m.value == want == mode_of_header(hdr)
        assert levels_of_header(hdr[0]) == 2
    # malformed config-B headers: AC with pad bits above its 4 flags, xwide without a count or with pad bits 4 .. 9 set
    for b0, padfield in ((2, pad | 0x10), (0xE9, pad), (0xE9, pad | 0x20 | (3 << 10))):
        hdr = bytes([b0, h1, w1]) + bytes(12) + int(padfield).to_bytes(2, "little")
        m = C.c_int(-1)
        assert L.llicti_header_mode((C.c_uint8 * 17).from_buffer_copy(hdr), C.byref(m)) == _lib.EFORMAT
        with pytest.raises(ValueError):
            mode_of_header(hdr)


def test_llic_file_holds_config_b_containers(tmp_path):
    """The .llic file stores its segment count: a config-B bytestream_list (3 rows, 22 segments) round-trips unchanged."""
    from llicti_amd import fileio
    from llicti_amd.codec import bytestream_list_to_container, container_to_bytestream_list
    rng = np.random.default_rng(3)
    segs = [bytes([2, 8, 8]), bytes(12), bytes([0, 0]), bytes(rng.integers(0, 256, 192, dtype=np.uint8))]
    segs += [bytes(rng.integers(0, 256, int(n), dtype=np.uint8)) for n in rng.integers(1, 60, 18)]
    bl = [segs[:4] + [b""] * 5, segs[4:13], segs[13:22]]
    f = tmp_path / "b.llic"
    fileio.write_llic(str(f), bl)
    assert fileio.read_llic(str(f)) == bl
    buf, seg = bytestream_list_to_container(bl)
    assert seg.shape == (49,) and seg[22:].sum() == 0 and int(seg.sum()) == buf.size
    assert container_to_bytestream_list(buf, seg) == bl
