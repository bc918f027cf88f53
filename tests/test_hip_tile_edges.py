"""GPU tests of the band CNN and the table kernel at every tile edge (run with -m gpu on an MI355X).

The band CNN stages a tile's input halo through a fast path (halo strictly inside the band grid, per-lane offsets precomputed; the
mixed-size RAGGED form recomputes them per piece) or a border path (clamp + lazyDWT's odd-edge pad), in three tile forms (16, 8, 4 rows)
and two instantiations (equal sizes, RAGGED).  The sweep shapes (helpers.SWEEP_SHAPES) put tiles on the last row / column the fast path
accepts and the first it refuses, in every form, at both parities of the level grid; every output is held BIT-EQUAL to the CPU oracle and
within a rigorous bound of a float64 restatement of the model (tests/ref64.py), which shares neither packing nor numerics code with the two."""
import numpy as np
import pytest

import ref64
from conftest import load_state_dict
from helpers import SWEEP_SHAPES, all_tile_edge_classes, make_image, tile_edge_classes

pytestmark = pytest.mark.gpu

TILE_ROWS = (16, 8, 4, 0)          # the three forms forced, then the automatic choice


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def codecs(torch_mod):
    from llicti_amd.codec import HipCodec
    cache = {}

    def get(wname):
        if wname not in cache:
            c = HipCodec("cuda:0")
            c.load_state_dict(load_state_dict(wname))
            cache[wname] = c
        return cache[wname]
    yield get
    for c in cache.values():
        c.set_tuning("cnn_tile_rows", 0)
        c.close()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _sweep_images(H, W, B, seed0):
    return np.stack([make_image(("smooth", "noise")[i % 2], H, W, seed0 + i) for i in range(B)])


def test_sweep_shapes_cover_every_tile_edge_class():
    """The coverage the tests below rely on, computed from the level geometry: all 72 classes (tile form x last-accepted / first-refused row x
    fast-edge / border-edge / interior column x parity of Hl and Wl), at levels 0-2 -- an edit of the list cannot drop one silently."""
    from oracle import oracle as orc
    got = set()
    for H, W in SWEEP_SHAPES:
        got |= tile_edge_classes(H, W)
        for lvl in range(3):                                        # (the helper's geometry is the oracle's)
            Hl, Wl, h, w, _, _ = orc.level_geom(H, W, lvl)
            assert ref64.level_geom(H, W, lvl) == (Hl, Wl, h, w)
    assert got == all_tile_edge_classes(), sorted(all_tile_edge_classes() - got)


@pytest.mark.parametrize("wname", ["trainedlike", "rand1337"])
def test_band_params_tile_edges_bitexact_and_float64(torch_mod, codecs, oracle_weights, wname):
    """Equal-size kernel (llicti_band_params_f32), B = 2 images of different content per sweep shape, every tile form and the automatic
    choice, all 5 levels x 3 bands: the 60 parameters BIT-EQUAL to the oracle's, and within cnn_error_bound of the float64 CNN."""
    from oracle import oracle as orc
    torch = torch_mod
    c = codecs(wname)
    W_o = oracle_weights(wname)
    sd = load_state_dict(wname)
    worst = 0.0
    try:
        for k, (H, W) in enumerate(SWEEP_SHAPES):
            rgb = _sweep_images(H, W, 2, 900 + 10 * k)
            planes, fplanes, _ = c.lift(_dev(torch, rgb))
            p_host = planes.cpu().numpy()
            fp_host = fplanes.cpu().numpy()
            ref = {(b, lvl, band): orc.band_params(p_host[b], lvl, band, W_o) for b in range(2) for lvl in range(5) for band in range(3)}
            for rows in TILE_ROWS:
                c.set_tuning("cnn_tile_rows", rows)
                for lvl in range(5):
                    for band in range(3):
                        got = c.params60(c.band_params(fplanes, lvl, band)).cpu().numpy()
                        for b in range(2):
                            r = ref[(b, lvl, band)]
                            assert got[b].shape == r.shape
                            if not np.array_equal(got[b].view(np.uint32), r.view(np.uint32)):
                                bad = np.argwhere((got[b] != r).any(-1))
                                pytest.fail(f"{H}x{W} image {b} rows {rows} level {lvl} band {band}: {len(bad)} positions differ from the oracle, "
                                            f"first {bad[:4].tolist()}, max |d| {np.abs(got[b] - r).max():.3g}")
                            if rows == 0:
                                r64 = ref64.band_params64(fp_host[b], lvl, band, sd)
                                bnd = ref64.cnn_error_bound(fp_host[b], lvl, band, sd)
                                q = (np.abs(got[b] - r64) / bnd).max()
                                assert q <= 1.0, (H, W, b, lvl, band, q)
                                worst = max(worst, q)
    finally:
        c.set_tuning("cnn_tile_rows", 0)
    print(f"{wname}: largest |kernel - float64| / bound of the CNN outputs: {worst:.3g}")


def test_band_params_ragged_tile_edges(torch_mod, codecs, oracle_weights):
    """RAGGED form: the 16 sweep shapes in ONE mixed-size batch through llicti_encode_images_v (xwide rANS, 2 streams: a fixed count every
    shape accepts), for every tile form: each image's container is the oracle's byte for byte, the batch decodes losslessly on a poisoned
    workspace, and the CNN outputs of the last launch (level 0, band x10) of the encoder and of the decoder, read out of the workspace, are
    BIT-EQUAL to the equal-size kernel's on that image alone."""
    from llicti_amd.codec import MODE_RANS, container_to_bytestream_list
    from oracle import oracle as orc
    torch = torch_mod
    wname = "trainedlike"
    c = codecs(wname)
    W_o = oracle_weights(wname)
    mode = MODE_RANS(2, wide=2)
    rgbs = [make_image(("smooth", "noise")[k % 2], H, W, 1300 + k) for k, (H, W) in enumerate(SWEEP_SHAPES)]
    Hs, Ws = [H for H, _ in SWEEP_SHAPES], [W for _, W in SWEEP_SHAPES]
    want = [orc.encode_image_rans(rgb, W_o, 2, 2) for rgb in rgbs]
    flat = _dev(torch, np.concatenate([r.reshape(-1) for r in rgbs]))
    try:
        for rows in TILE_ROWS:
            c.set_tuning("cnn_tile_rows", rows)
            single = []
            for rgb in rgbs:                                           # the equal-size kernel's level-0 / band-2 planes of each image alone
                _, fpl, _ = c.lift(_dev(torch, rgb[None]))
                single.append(c.band_params(fpl, 0, 2)[0].reshape(64, -1).clone())
            cont, seg = c.encode_v(flat, Hs, Ws, mode)
            c.check()
            cont_h, seg_h = cont.cpu().numpy(), seg.cpu().numpy()
            for b in range(len(rgbs)):
                assert container_to_bytestream_list(cont_h[b], seg_h[b]) == want[b], (rows, Hs[b], Ws[b])
            used = [p for p in range(64) if p % 16 != 15]              # (plane 15 of a head does not exist: never written)
            for what in ("encode", "decode"):
                if what == "decode":
                    c.poison_workspace()
                    rec = c.decode_v(cont, seg, Hs, Ws, mode).cpu().numpy()
                    c.check()
                    assert not c.image_status(len(rgbs)).any()
                    pos = 0
                    for b, rgb in enumerate(rgbs):
                        n = rgb.size
                        assert np.array_equal(rec[pos:pos + n].reshape(rgb.shape), rgb), (rows, b)
                        pos += n
                for b in range(len(rgbs)):
                    got = c.last_params_v(Hs, Ws, mode, b)
                    assert torch.equal(got[used], single[b][used]), (what, rows, Hs[b], Ws[b])
    finally:
        c.set_tuning("cnn_tile_rows", 0)


def _table_shapes():
    """Sweep shapes whose stages' row counts hc * wc take every residue mod 8 (the table kernel works in runs of 8 rows per wavefront); the
    sweep's stages miss residues 5 and 7 (both dimensions odd), which 65 x 91 adds."""
    from llicti_amd._lib import level_geom
    chosen, seen = [], set()
    for H, W in SWEEP_SHAPES + [(65, 91)]:
        res = {level_geom(H, W, lvl, band)[-2] * level_geom(H, W, lvl, band)[-1] % 8 for lvl in range(5) for band in range(3)}
        if not res <= seen:
            chosen.append((H, W))
            seen |= res
    assert seen == set(range(8)), seen
    return chosen


def test_cdf_tables_every_row_tile_edges(torch_mod, codecs, oracle_weights):
    """llicti_cdf_u16, every row of every stage and colour, both row strides (512 / 264 and the tight multiple of 8), on sweep shapes whose row
    counts take every residue mod 8: each row equal to the oracle's and within the float64 tolerance; the padding entries 0xFFFF."""
    from llicti_amd._lib import level_geom
    from oracle import oracle as orc
    torch = torch_mod
    worst = 0.0
    for k, (H, W) in enumerate(_table_shapes()):
        wname = ("trainedlike", "rand1337")[k % 2]
        c = codecs(wname)
        W_o = oracle_weights(wname)
        rgb = make_image("smooth", H, W, 1700 + k)
        planes, fplanes, mm = c.lift(_dev(torch, rgb[None]))
        p_host, mm_ref = orc.lift(rgb)
        for lvl in range(5):
            for band in range(3):
                params = c.band_params(fplanes, lvl, band)
                par = orc.band_params(p_host, lvl, band, W_o)
                assert np.array_equal(c.params60(params)[0].cpu().numpy().view(np.uint32), par.view(np.uint32))
                *_, hc, wc = level_geom(H, W, lvl, band)
                a, b = ref64.TARGET[band]
                rows_, cols_ = np.arange(a << lvl, H, 2 << lvl), np.arange(b << lvl, W, 2 << lvl)
                assert (len(rows_), len(cols_)) == (hc, wc)
                P = par[:hc, :wc].reshape(-1, 60)
                tg = p_host[:, rows_][:, :, cols_].reshape(3, -1).astype(np.float32) / np.float32(255)
                for clr in range(3):
                    minv = -127 if clr == 0 else int(mm_ref[clr])
                    maxv = 128 if clr == 0 else int(mm_ref[3 + clr])
                    Lp = maxv - minv + 2
                    want = orc.cdf_rows(P, clr, tg[0], tg[1], minv, maxv)
                    ent, tol = ref64.cdf_entries64(P, clr, tg[0], tg[1], minv, maxv)
                    for stride in ((264, 512) if clr == 0 else (512, max(8, (Lp + 7) // 8 * 8))):
                        tab = c.cdf_tables(planes, params, mm, lvl, band, clr, row_stride=stride)[0].cpu().numpy().view(np.uint16)
                        assert tab.shape == (hc * wc, stride)
                        if not np.array_equal(tab[:, :Lp], want):
                            bad = np.argwhere((tab[:, :Lp] != want).any(1)).ravel()
                            pytest.fail(f"{H}x{W} level {lvl} band {band} colour {clr} stride {stride}: rows {bad[:8].tolist()} of {hc * wc} differ from the oracle")
                        assert (tab[:, Lp:] == 0xFFFF).all(), (H, W, lvl, band, clr, stride)
                        q = (np.abs(ref64.wrap_diff(tab[:, :Lp], ent)) / tol).max()
                        assert q <= 1.0, (H, W, lvl, band, clr, stride, q)
                        worst = max(worst, q)
    print(f"largest |kernel - float64| / tolerance of the table entries: {worst:.3g}")


@pytest.mark.parametrize("wname", ["trainedlike", "rand1337"])
def test_selfinfo_tile_edges_float64(torch_mod, codecs, wname):
    """selfinfo (and forward_selfinfo, which chains the float lift, the CNN and it) at the sweep shapes: within selfinfo64's tolerance of the
    float64 self-information of the kernel's own CNN outputs."""
    torch = torch_mod
    c = codecs(wname)
    worst = 0.0
    for k, (H, W) in enumerate(SWEEP_SHAPES[k0] for k0 in range(0, 16, 3)):
        rgb = make_image(("smooth", "noise")[k % 2], H, W, 2100 + k)
        x = _dev(torch, rgb[None])
        fpl = c.lift_train(x)
        fp_host = fpl[0].cpu().numpy()
        infos = c.forward_selfinfo(x)
        for lvl in range(5):
            for band in range(3):
                params = c.band_params(fpl, lvl, band)
                si = c.selfinfo(fpl, params, lvl, band)
                assert torch.equal(si, infos[lvl][:, 3 * band:3 * band + 3])
                ref, tol = ref64.selfinfo64(fp_host, lvl, band, c.params60(params)[0].cpu().numpy())
                q = (np.abs(si[0].cpu().numpy() - ref) / tol).max()
                assert q <= 1.0, (H, W, lvl, band, q)
                worst = max(worst, q)
    print(f"{wname}: largest |kernel - float64| / tolerance of the self-information: {worst:.3g}")


def test_auto_batch_mixing_fixed_and_auto_stream_counts(torch_mod, codecs):
    """Container "auto" on [2160x3840, 768x512]: the large image gets a fixed 64 xwide streams, the small one an encoder-picked count, in ONE
    call.  Each container equals the one its image gets in a call of its own, and the batch decodes losslessly."""
    from llicti_amd.codec import auto_modes, image_mode
    torch = torch_mod
    c = codecs("trainedlike")
    sizes = [(2160, 3840), (512, 768)]
    modes = auto_modes(sizes)
    assert modes == [image_mode(h, w, True) for h, w in sizes] and len({m & 0x10000 for m in modes}) == 2
    rgbs = [make_image("smooth", h, w, 2500 + i) for i, (h, w) in enumerate(sizes)]
    Hs, Ws = [h for h, _ in sizes], [w for _, w in sizes]
    cont, seg = c.encode_v(_dev(torch, np.concatenate([r.reshape(-1) for r in rgbs])), Hs, Ws, modes)
    c.check()
    cont_h, seg_h = cont.cpu().numpy(), seg.cpu().numpy()
    for b, rgb in enumerate(rgbs):
        c1, s1 = c.encode(_dev(torch, rgb[None]), mode=modes[b])
        c.check()
        n = int(seg_h[b].sum())
        assert np.array_equal(seg_h[b], s1[0].cpu().numpy()), b
        assert np.array_equal(cont_h[b, :n], c1[0, :n].cpu().numpy()), b
    dm = c.container_modes(cont)
    assert dm[0] == modes[0]
    c.poison_workspace()
    rec = c.decode_v(cont, seg, Hs, Ws, dm).cpu().numpy()
    c.check()
    assert not c.image_status(2).any()
    pos = 0
    for rgb in rgbs:
        assert np.array_equal(rec[pos:pos + rgb.size].reshape(rgb.shape), rgb)
        pos += rgb.size
