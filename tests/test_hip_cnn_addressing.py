"""GPU tests of the band CNN's addressing (run with -m gpu on an MI355X): the LDS reads of the tile loop take base register + offset field
(DESIGN.md section 8, round 10), and the params stores address a batch's buffer with 64 bits.

One tile exercises every weight, bias and input-fragment read; what can go wrong beyond that is the stores' addressing across images, heads,
tile rows and overhangs.  Every HIP `band_params` output is held BIT-EQUAL to the CPU oracle (the `_check` pattern of
tests/test_hip_cnn_layer0_operands.py), bands 0-2, the 16-, 8- and 4-row forms, config A and config B:
  (a) a batch of 3 different images of 33 x 65 (grid 17 x 33: one tile plus a one-row and a one-column overhang), all three compared:
      image index > 0, partial stores;
  (b) a batch of 2 images of 64 x 96 (grid 32 x 48: two tile rows of the 16-row form, one and a half tile columns);
  (c) grids smaller than a tile: 3 x 5 (level 3 of 40 x 72; config A) and 8 x 8 (level 1 of 32 x 32, config B's smallest);
  (d) one mixed-size call holding 33 x 65 and 32 x 96, outputs through last_params_v.  Band 2 of level 0 only: the mixed-size kernels run inside
      whole-batch calls alone (no kernel-level entry point takes images of different sizes), and last_params_v reads back what such a call
      leaves in its workspace: the outputs of its LAST CNN launch -- level 0, band 2.  Bands 0 and 1 of the mixed-size form
      are held by the call's containers, which tests/test_hip_cnn_layer0_operands.py compares byte for byte with the oracle's;
  (e) one equal-size call whose params buffer passes 4 GiB: 1,025 images of 256 x 256 at 4 MiB of level-0 parameters each (the smallest such
      batch of that size), band 2; image 0 and the last image against the oracle -- the stores' 64-bit addresses."""
import numpy as np
import pytest

from conftest import load_state_dict
from helpers import make_image
from test_hip_border_staging import padded_to_88

pytestmark = pytest.mark.gpu

TILE_ROWS = (16, 8, 4)
# (H, W, level, band grid, images)
CASE_A = (33, 65, 0, (17, 33), 3)
CASE_B = (64, 96, 0, (32, 48), 2)
CASE_C_A = (40, 72, 3, (3, 5), 2)
CASE_C_B = (32, 32, 1, (8, 8), 2)


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
        for k, (H, W, lvl, grid, B) in enumerate(cases):
            assert orc.level_geom(H, W, lvl)[2:4] == grid
            rgb = np.stack([make_image(("noise", "smooth")[(k + b) % 2], H, W, seed0 + 10 * k + b) for b in range(B)])
            planes, fplanes, _ = c.lift(_dev(torch, rgb))
            p_host = planes.cpu().numpy()
            for band in range(3):
                ref = np.stack([orc.band_params(p_host[b], lvl, band, W_o) for b in range(B)])
                for rows in TILE_ROWS:
                    c.set_tuning("cnn_tile_rows", rows)
                    got = c.params60(c.band_params(fplanes, lvl, band)).cpu().numpy()
                    assert got.shape == ref.shape
                    if not np.array_equal(got.view(np.uint32), ref.view(np.uint32)):
                        bad = np.argwhere((got != ref).any(-1))
                        pytest.fail(f"{B} x {H}x{W} level {lvl} (grid {grid}) band {band} rows {rows}: {len(bad)} positions differ from the oracle, "
                                    f"first (image, row, column) {bad[:4].tolist()}, max |d| {np.abs(got - ref).max():.3g}")
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


@pytest.fixture(scope="module")
def codec_b(torch_mod):
    """config B and the oracle's weights for it: the oracle's CNN is 88 wide, a 60-wide head runs through it zero-padded (the same fmaf chain)."""
    from llicti_amd.codec import HipCodec
    from llicti_amd.weights import pack_state_dict
    from oracle import oracle as orc
    sd = load_state_dict("b_trainedlike")
    c = HipCodec("cuda:0")
    c.set_model(60, 2)
    c.load_state_dict(sd)
    yield c, orc.Weights(padded_to_88(pack_state_dict(sd)))
    c.set_tuning("cnn_tile_rows", 0)
    c.close()


def test_config_a_batches_bitexact(torch_mod, codec_a, oracle_weights):
    """cases (a), (b), (c)"""
    _check(torch_mod, codec_a, oracle_weights("trainedlike"), [CASE_A, CASE_B, CASE_C_A], 9400)


def test_config_b_batches_bitexact(torch_mod, codec_b):
    """cases (a), (b), (c)"""
    c, W_o = codec_b
    _check(torch_mod, c, W_o, [CASE_A, CASE_B, CASE_C_B], 9500)


def _check_mixed(torch, c, W_o, mode, seed0):
    from oracle import oracle as orc
    sizes = [(33, 65), (32, 96)]
    rgbs = [make_image(("noise", "smooth")[k % 2], H, W, seed0 + k) for k, (H, W) in enumerate(sizes)]
    Hs, Ws = [H for H, _ in sizes], [W for _, W in sizes]
    want = [orc.band_params(orc.lift(rgb)[0], 0, 2, W_o).reshape(-1, 60) for rgb in rgbs]
    flat = _dev(torch, np.concatenate([r.reshape(-1) for r in rgbs]))
    try:
        for rows in TILE_ROWS:
            c.set_tuning("cnn_tile_rows", rows)
            c.encode_v(flat, Hs, Ws, mode)
            c.check()
            for b, (H, W) in enumerate(sizes):
                h, w = orc.level_geom(H, W, 0)[2:4]
                got = c.params60(c.last_params_v(Hs, Ws, mode, b).view(1, 64, h, w))[0].cpu().numpy().reshape(-1, 60)
                assert np.array_equal(got.view(np.uint32), want[b].view(np.uint32)), (rows, H, W, int((got != want[b]).any(-1).sum()))
    finally:
        c.set_tuning("cnn_tile_rows", 0)


def test_config_a_mixed_size_call_bitexact(torch_mod, codec_a, oracle_weights):
    """case (d)"""
    from llicti_amd.codec import MODE_RANS
    _check_mixed(torch_mod, codec_a, oracle_weights("trainedlike"), MODE_RANS(2, wide=2), 9600)


def test_config_b_mixed_size_call_bitexact(torch_mod, codec_b):
    """case (d), config B"""
    from llicti_amd.codec import auto_modes
    c, W_o = codec_b
    _check_mixed(torch_mod, c, W_o, auto_modes([(33, 65), (32, 96)], nlevels=2), 9700)


def test_params_buffer_beyond_4gib_bitexact(torch_mod, codec_a, oracle_weights):
    """case (e).  The images between the first and the last repeat three others, so every image's stores are checked: against the oracle at both
    ends of the buffer, against the first images' on the device in between."""
    from oracle import oracle as orc
    torch, c, W_o = torch_mod, codec_a, oracle_weights("trainedlike")
    B, H, W = 1025, 256, 256
    base = np.stack([make_image(("noise", "smooth", "noise", "smooth")[k], H, W, 9800 + k) for k in range(4)])
    idx = np.arange(B) % 3
    idx[-1] = 3
    rgb = _dev(torch, base)[torch.from_numpy(idx).to("cuda:0")].contiguous()
    planes, fplanes, _ = c.lift(rgb)
    del rgb
    out = c.band_params(fplanes, 0, 2)
    assert out.numel() * 4 > 1 << 32 and (B - 1) * out[0].numel() * 4 <= 1 << 32      # the smallest such batch; the last image starts at 4 GiB
    for b in (0, B - 1):
        ref = orc.band_params(planes[b].cpu().numpy(), 0, 2, W_o)
        got = c.params60(out[b:b + 1]).cpu().numpy()[0]
        bad = np.argwhere((got.view(np.uint32) != ref.view(np.uint32)).any(-1))
        assert len(bad) == 0, f"image {b}: {len(bad)} positions differ from the oracle, first {bad[:4].tolist()}"
    bits = out.view(torch.int32).view(B, 4, 16, -1)[:, :, :15]           # (a head's 16th plane is never written)
    groups = bits[:1023].unflatten(0, (341, 3))                           # images 0 .. 1022: 341 times the first three
    assert bool((groups == groups[:1]).all()), "an image between the ends differs from its first copy"
    assert bool((bits[1023] == bits[0]).all())
