"""GPU tests of the band CNN's BORDER staging path (run with -m gpu on an MI355X), for the cases tests/test_hip_tile_edges.py does not single out.

A border tile's pieces are staged in two ways (band_cnn.hpp, lambda `stage`): pieces whose two rows lie inside the grid take the interior
formula with per-phase clamped-column offsets, the others the general clamping formula, one by one; a tile that reaches the last column of
a grid with odd Wl sends all its pieces the second way.  Every output here is held BIT-EQUAL to the CPU oracle:
  - config B (band_params_h60_kernel) on four sweep shapes, every tile form.  The oracle's CNN is 88 wide; a 60-wide head is run through it
    zero-padded to 88 channels (padded hidden channels are relu(0 + 0 x ...) = 0 and add fmaf(0, 0, acc) = acc to the chains behind them, in
    the place where the kernel's own padding to 64 rows adds the same), so it is the oracle's fmaf chain that the kernel is compared with;
  - grids narrower than one tile (32 columns) and shorter than one tile (16 / 8 / 4 rows), where a tile clamps on both sides at once, at both
    parities of Hl and Wl;
  - tiles that overhang the grid by all but one row / column (h = 17 under 16-row tiles, w = 33);
  - one mixed-size call (RAGGED form) with such images next to a 512 x 768 one.
The shapes are small: the oracle's part of this file runs in about ten seconds on a CPU."""
import numpy as np
import pytest

from conftest import load_state_dict
from helpers import SWEEP_SHAPES, make_image

pytestmark = pytest.mark.gpu

TILE_ROWS = (16, 8, 4, 0)          # the three forms forced, then the automatic choice
B_SHAPES = [SWEEP_SHAPES[0], SWEEP_SHAPES[5], SWEEP_SHAPES[10], SWEEP_SHAPES[15]]      # 67x133, 68x134, 69x195, 70x196: every parity of Hl and Wl
# level-0 grids 17 x 17 .. 24 x 31 (narrower than a tile; levels 1-4: shorter than every tile form too, down to 1 x 1), Hl / Wl odd and even
SMALL_SHAPES = [(33, 33), (34, 48), (47, 34), (48, 61), (37, 62)]
# h = 17 and / or w = 33 at level 0: the second tile row / column holds ONE row / column of the grid (and 9 = 8 + 1, 5 = 4 + 1 rows at levels 1, 2)
OVERHANG_SHAPES = [(33, 65), (34, 66), (33, 130), (66, 65)]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def padded_to_88(packed):
    """pack_state_dict() of a 60-wide model -> the same model as an 88-wide one: channels 60..87 of every head have zero weights and biases."""
    out = {}
    for b, d in packed.items():
        hw, K0 = int(d["head"]), int(d["K0"])
        assert hw == 60
        w0, b0 = np.zeros((4 * 88, K0), np.float32), np.zeros(4 * 88, np.float32)
        w1, b1 = np.zeros((4 * 88, 88), np.float32), np.zeros(4 * 88, np.float32)
        w2 = np.zeros((60, 88), np.float32)
        for g in range(4):
            w0[g * 88:g * 88 + hw] = d["w0"][g * hw:(g + 1) * hw]
            b0[g * 88:g * 88 + hw] = d["b0"][g * hw:(g + 1) * hw]
            w1[g * 88:g * 88 + hw, :hw] = d["w1"][g * hw:(g + 1) * hw]
            b1[g * 88:g * 88 + hw] = d["b1"][g * hw:(g + 1) * hw]
        w2[:, :hw] = d["w2"]
        out[b] = {"K0": K0, "head": 88, "w0": w0, "b0": b0, "w1": w1, "b1": b1, "w2": w2, "b2": np.ascontiguousarray(d["b2"], dtype=np.float32)}
    return out


def _check_band_params(torch, c, W_o, shapes, levels, seed0):
    """llicti_band_params_f32 on B = 2 images per shape, every tile form, the given levels x 3 bands: BIT-EQUAL to the oracle's"""
    from oracle import oracle as orc
    try:
        for k, (H, W) in enumerate(shapes):
            rgb = np.stack([make_image(("smooth", "noise")[(k + i) % 2], H, W, seed0 + 10 * k + i) for i in range(2)])
            planes, fplanes, _ = c.lift(_dev(torch, rgb))
            p_host = planes.cpu().numpy()
            for lvl in levels:
                for band in range(3):
                    ref = [orc.band_params(p_host[b], lvl, band, W_o) for b in range(2)]
                    for rows in TILE_ROWS:
                        c.set_tuning("cnn_tile_rows", rows)
                        got = c.params60(c.band_params(fplanes, lvl, band)).cpu().numpy()
                        for b in range(2):
                            assert got[b].shape == ref[b].shape
                            if not np.array_equal(got[b].view(np.uint32), ref[b].view(np.uint32)):
                                bad = np.argwhere((got[b] != ref[b]).any(-1))
                                pytest.fail(f"{H}x{W} image {b} rows {rows} level {lvl} band {band}: {len(bad)} positions differ from the oracle, "
                                            f"first {bad[:4].tolist()}, max |d| {np.abs(got[b] - ref[b]).max():.3g}")
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


@pytest.mark.parametrize("wname", ["rand1337", "trainedlike"])
def test_config_b_border_tiles_bitexact(torch_mod, wname):
    """band_params_h60_kernel, both levels of config B, on four sweep shapes (every tile-edge class of tests/helpers.py at both parities)."""
    from llicti_amd.codec import HipCodec
    from llicti_amd.weights import pack_state_dict
    from oracle import oracle as orc
    sd = load_state_dict(f"b_{wname}")
    W_o = orc.Weights(padded_to_88(pack_state_dict(sd)))
    c = HipCodec("cuda:0")
    try:
        c.set_model(60, 2)
        c.load_state_dict(sd)
        _check_band_params(torch_mod, c, W_o, B_SHAPES, (0, 1), 3100)
    finally:
        c.close()


def test_grids_smaller_than_a_tile_bitexact(torch_mod, codec_a, oracle_weights):
    """Every tile clamps on the left AND on the right (w < 32), and at the coarser levels at the top and the bottom too (h below the tile rows)."""
    from oracle import oracle as orc
    for H, W in SMALL_SHAPES:
        _, _, h, w, _, _ = orc.level_geom(H, W, 0)
        assert w < 32 and orc.level_geom(H, W, 2)[2] < 16
    assert {orc.level_geom(H, W, 0)[0] % 2 for H, W in SMALL_SHAPES} == {0, 1} and {orc.level_geom(H, W, 0)[1] % 2 for H, W in SMALL_SHAPES} == {0, 1}
    _check_band_params(torch_mod, codec_a, oracle_weights("trainedlike"), SMALL_SHAPES, range(5), 3300)


def test_tiles_overhanging_by_most_of_a_tile_bitexact(torch_mod, codec_a, oracle_weights):
    from oracle import oracle as orc
    assert {orc.level_geom(H, W, 0)[2] for H, W in OVERHANG_SHAPES} == {17, 33} and {orc.level_geom(H, W, 0)[3] for H, W in OVERHANG_SHAPES} == {33, 65}
    _check_band_params(torch_mod, codec_a, oracle_weights("trainedlike"), OVERHANG_SHAPES, range(5), 3500)


def test_mixed_size_call_with_small_grids_next_to_a_full_size_image(torch_mod, codec_a, oracle_weights):
    """RAGGED form, every tile form: small-grid and overhanging images beside a 512 x 768 one in ONE llicti_encode_images_v call.  The small
    images' containers are the oracle's byte for byte; every image's CNN outputs of the last launch (level 0, band x10), encoder and decoder,
    are BIT-EQUAL to the oracle's; the batch decodes losslessly on a poisoned workspace."""
    from llicti_amd.codec import MODE_RANS, container_to_bytestream_list
    from oracle import oracle as orc
    torch = torch_mod
    c = codec_a
    W_o = oracle_weights("trainedlike")
    mode = MODE_RANS(2, wide=2)
    sizes = [(33, 65), (512, 768), (34, 48), (47, 34), (66, 65)]
    rgbs = [make_image(("smooth", "noise")[k % 2], H, W, 3700 + k) for k, (H, W) in enumerate(sizes)]
    Hs, Ws = [H for H, _ in sizes], [W for _, W in sizes]
    want_bytes = {b: orc.encode_image_rans(rgb, W_o, 2, 2) for b, rgb in enumerate(rgbs) if rgb.shape[1] < 512}
    want_par = []
    for rgb in rgbs:
        par = orc.band_params(orc.lift(rgb)[0], 0, 2, W_o)                # [h, w, 60]
        want_par.append(par.reshape(-1, 60))
    flat = _dev(torch, np.concatenate([r.reshape(-1) for r in rgbs]))
    try:
        for rows in TILE_ROWS:
            c.set_tuning("cnn_tile_rows", rows)
            cont, seg = c.encode_v(flat, Hs, Ws, mode)
            c.check()
            cont_h, seg_h = cont.cpu().numpy(), seg.cpu().numpy()
            for b, want in want_bytes.items():
                assert container_to_bytestream_list(cont_h[b], seg_h[b]) == want, (rows, sizes[b])
            for what in ("encode", "decode"):
                if what == "decode":
                    c.poison_workspace()
                    rec = c.decode_v(cont, seg, Hs, Ws, mode).cpu().numpy()
                    c.check()
                    assert not c.image_status(len(rgbs)).any()
                    pos = 0
                    for b, rgb in enumerate(rgbs):
                        assert np.array_equal(rec[pos:pos + rgb.size].reshape(rgb.shape), rgb), (rows, b)
                        pos += rgb.size
                for b, (H, W) in enumerate(sizes):
                    _, _, h, w, _, _ = orc.level_geom(H, W, 0)
                    got = c.params60(c.last_params_v(Hs, Ws, mode, b).view(1, 64, h, w))[0].cpu().numpy().reshape(-1, 60)
                    assert np.array_equal(got.view(np.uint32), want_par[b].view(np.uint32)), (what, rows, H, W)
    finally:
        c.set_tuning("cnn_tile_rows", 0)
