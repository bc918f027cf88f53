"""The crop rule tests/test_hip_large.py stands on, held on the CPU oracle where the whole image is affordable: the band CNN is local, so a crop
whose origin is a multiple of 32 and which runs to the image's bottom-right corner (true borders and odd-edge pad included), or a 32-aligned
crop from its top-left corner, has band_params BIT-EQUAL to the whole image's from margin 2 inwards of every cut side -- at all 5 levels and
3 bands, for both weight sets.  The coder's pairs follow, once the crop is given the IMAGE's min/max.  (helpers.crop_windows)"""
import numpy as np
import pytest

from helpers import crop_windows, make_image


@pytest.fixture(scope="module")
def orc_mod():
    from oracle import oracle as orc
    orc.build()
    return orc


def _full(orc, W_o, img):
    planes, mm = orc.lift(img)
    return planes, mm, {(lvl, band): orc.band_params(planes, lvl, band, W_o) for lvl in range(5) for band in range(3)}


_cache = {}


@pytest.mark.parametrize("wname", ["rand1337", "trainedlike"])
@pytest.mark.parametrize("H,W", [(416, 480), (417, 479)])
def test_crop_params_and_pairs_equal_the_whole_images(orc_mod, oracle_weights, H, W, wname):
    orc = orc_mod
    W_o = oracle_weights(wname)
    img = make_image("noise", H, W, 21)
    planes, mm, full = _full(orc, W_o, img)
    y0, x0 = (H - 192) // 32 * 32, (W - 192) // 32 * 32           # a 192-pixel crop (192 .. 223 with the odd edge) to the bottom-right corner ...
    for (cy, cx, ch, cw) in ((y0, x0, None, None), (0, 0, 192, 192)):      # ... and the top-left 192x192
        crop, wins = crop_windows(img, cy, cx, ch, cw, margin=2)
        assert crop.shape[1] >= 192 and crop.shape[2] >= 192
        cplanes, _ = orc.lift(np.ascontiguousarray(crop))
        assert np.array_equal(cplanes, planes[:, cy:cy + crop.shape[1], cx:cx + crop.shape[2]])
        for lvl in range(5):
            fr, fc, cr, cc = wins[lvl]
            for band in range(3):
                par_c = orc.band_params(cplanes, lvl, band, W_o)
                a, b = full[(lvl, band)][fr, fc], par_c[cr, cc]
                assert a.shape == b.shape and a.size > 0
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (lvl, band, cy, cx)
                if cy:      # (not vacuous: the crop's own first row, computed over a replicated edge instead of the image's pixels, differs)
                    assert not np.array_equal(full[(lvl, band)][fr.start - 2, fc], par_c[0, cc]), (lvl, band)
            # the coder's pairs of the crop, given the IMAGE's min/max, against the image's own: level 0 and the coarsest level, band x11
            for lv in (0, 4):
                if lv != lvl:
                    continue
                _, _, gh, gw, padH, padW = orc.level_geom(H, W, lvl)
                _, _, ghc, gwc, padHc, padWc = orc.level_geom(crop.shape[1], crop.shape[2], lvl)
                hc_f, wc_f, hc_c, wc_c = gh - padH, gw - padW, ghc - padHc, gwc - padWc      # band 0 codes the grid less its padded row / column
                for clr in range(3):
                    lo_f, hi_f, sym_f = orc.stream_pairs(planes, mm, lvl, 0, clr, full[(lvl, 0)])
                    lo_c, hi_c, sym_c = orc.stream_pairs(cplanes, mm, lvl, 0, clr, orc.band_params(cplanes, lvl, 0, W_o))
                    assert lo_f.size == hc_f * wc_f and lo_c.size == hc_c * wc_c
                    rr_f, rc_f = slice(fr.start, min(fr.stop, hc_f)), slice(fc.start, min(fc.stop, wc_f))
                    rr_c, rc_c = slice(cr.start, min(cr.stop, hc_c)), slice(cc.start, min(cc.stop, wc_c))
                    for f, c in ((lo_f, lo_c), (hi_f, hi_c), (sym_f, sym_c)):
                        assert np.array_equal(f.reshape(hc_f, wc_f)[rr_f, rc_f], c.reshape(hc_c, wc_c)[rr_c, rc_c]), (lvl, clr)
