"""GPU tests of the band CNN's layer-0 operand path (run with -m gpu on an MI355X): the input-tile fragment reads of a wave's two pixel tiles,
the 4x4x1 remainder path's reads of the same staged row, and the lane permutation that hands the remainder's channels to layer 1.

Every HIP `band_params` output here is held BIT-EQUAL to the CPU oracle, one image per call, bands 0-2, config A (band_params_kernel, with the
remainder path) and config B (band_params_h60_kernel, without), in the 16-, 8- and 4-row forms (the `cnn_tile_rows` tuning).  The band grids are
the smallest at which a changed fragment read or lane permutation can go wrong:
  - 3 x 5: smaller than a tile in both directions, and shorter than the 4-row form.  Images below 32 x 32 are refused (check_dims), so the grid
    is level 3 of a 40 x 72 image; config B has two levels, its smallest grid is 8 x 8 (level 1 of a 32 x 32 image);
  - 16 x 32: exactly one tile of the 16-row form (32 x 64 image, level 0);
  - 17 x 33: one tile plus a one-row and a one-column overhang (33 x 65);
  - 16 x 48: one and a half tiles wide (32 x 96).  The remainder path covers a wave's 32-pixel row as ONE run of eight pixel groups of four, across
    the 16-column boundary between the wave's two pixel tiles; in the second tile the groups on one side of that boundary hold grid positions
    and those on the other side lie outside the grid (clamped input, no store).
One mixed-size call (RAGGED form) holds the 17 x 33 and the 16 x 48 grid."""
import numpy as np
import pytest

from conftest import load_state_dict
from helpers import make_image
from test_hip_border_staging import padded_to_88

pytestmark = pytest.mark.gpu

TILE_ROWS = (16, 8, 4)
# (H, W, level) -> band grid
CASES_A = [(40, 72, 3, (3, 5)), (32, 64, 0, (16, 32)), (33, 65, 0, (17, 33)), (32, 96, 0, (16, 48))]
CASES_B = [(32, 32, 1, (8, 8)), (32, 64, 0, (16, 32)), (33, 65, 0, (17, 33)), (32, 96, 0, (16, 48))]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _check(torch, c, W_o, cases, seed0):
    from oracle import oracle as orc
    try:
        for k, (H, W, lvl, grid) in enumerate(cases):
            assert orc.level_geom(H, W, lvl)[2:4] == grid
            rgb = make_image(("noise", "smooth")[k % 2], H, W, seed0 + k)[None]
            planes, fplanes, _ = c.lift(_dev(torch, rgb))
            p_host = planes.cpu().numpy()[0]
            for band in range(3):
                ref = orc.band_params(p_host, lvl, band, W_o)
                for rows in TILE_ROWS:
                    c.set_tuning("cnn_tile_rows", rows)
                    got = c.params60(c.band_params(fplanes, lvl, band)).cpu().numpy()[0]
                    assert got.shape == ref.shape
                    if not np.array_equal(got.view(np.uint32), ref.view(np.uint32)):
                        bad = np.argwhere((got != ref).any(-1))
                        pytest.fail(f"{H}x{W} level {lvl} (grid {grid}) band {band} rows {rows}: {len(bad)} positions differ from the oracle, "
                                    f"first {bad[:4].tolist()}, max |d| {np.abs(got - ref).max():.3g}")
    finally:
        c.set_tuning("cnn_tile_rows", 0)


@pytest.fixture(scope="module")
def codec_a(torch_mod):
    from llicti_amd.codec import HipCodec
    c = HipCodec("cuda:0")
    c.load_state_dict(load_state_dict("trainedlike"))
    yield c
    c.set_tuning("cnn_tile_rows", 0)
    c.close()


def test_config_a_layer0_operands_bitexact(torch_mod, codec_a, oracle_weights):
    _check(torch_mod, codec_a, oracle_weights("trainedlike"), CASES_A, 9100)


def test_config_b_layer0_operands_bitexact(torch_mod):
    """The oracle's CNN is 88 wide: a 60-wide head runs through it zero-padded (tests/test_hip_border_staging.py: the same fmaf chain)."""
    from llicti_amd.codec import HipCodec
    from llicti_amd.weights import pack_state_dict
    from oracle import oracle as orc
    sd = load_state_dict("b_trainedlike")
    W_o = orc.Weights(padded_to_88(pack_state_dict(sd)))
    c = HipCodec("cuda:0")
    try:
        c.set_model(60, 2)
        c.load_state_dict(sd)
        _check(torch_mod, c, W_o, CASES_B, 9200)
    finally:
        c.close()


def test_mixed_size_call_layer0_operands_bitexact(torch_mod, codec_a, oracle_weights):
    """RAGGED form: the 17 x 33 and the 16 x 48 grid in ONE llicti_encode_images_v call, every tile form: containers byte for byte the oracle's,
    the CNN outputs of the last launch (level 0, band 2) BIT-EQUAL to the oracle's."""
    from llicti_amd.codec import MODE_RANS, container_to_bytestream_list
    from oracle import oracle as orc
    torch, c, W_o = torch_mod, codec_a, oracle_weights("trainedlike")
    mode = MODE_RANS(2, wide=2)
    sizes = [(33, 65), (32, 96)]
    rgbs = [make_image(("noise", "smooth")[k % 2], H, W, 9300 + k) for k, (H, W) in enumerate(sizes)]
    Hs, Ws = [H for H, _ in sizes], [W for _, W in sizes]
    want_bytes = [orc.encode_image_rans(rgb, W_o, 2, 2) for rgb in rgbs]
    want_par = [orc.band_params(orc.lift(rgb)[0], 0, 2, W_o).reshape(-1, 60) for rgb in rgbs]
    flat = _dev(torch, np.concatenate([r.reshape(-1) for r in rgbs]))
    try:
        for rows in TILE_ROWS:
            c.set_tuning("cnn_tile_rows", rows)
            cont, seg = c.encode_v(flat, Hs, Ws, mode)
            c.check()
            cont_h, seg_h = cont.cpu().numpy(), seg.cpu().numpy()
            for b, (H, W) in enumerate(sizes):
                assert container_to_bytestream_list(cont_h[b], seg_h[b]) == want_bytes[b], (rows, H, W)
                _, _, h, w, _, _ = orc.level_geom(H, W, 0)
                got = c.params60(c.last_params_v(Hs, Ws, mode, b).view(1, 64, h, w))[0].cpu().numpy().reshape(-1, 60)
                assert np.array_equal(got.view(np.uint32), want_par[b].view(np.uint32)), (rows, H, W)
    finally:
        c.set_tuning("cnn_tile_rows", 0)
