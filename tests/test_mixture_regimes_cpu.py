"""The adversarial mixture regimes (tests/mixture_regimes.py) on the CPU: the pinned rows reach the coder, the oracle round-trips every regime and
image in every container kind, the second reader of the rANS format (tests/ref_rans.py) agrees, and each image holds the symbol classes its
regime exists for -- as CONDITIONS with fixed minimum counts, so that tests/test_hip_mixture_regimes.py cannot quietly become a test of
ordinary content.  No GPU."""
import numpy as np
import pytest

import mixture_regimes as mr
import ref_rans as rr
from oracle import oracle as orc

MIN_OTHER, MIN_LAST = 64, 16          # symbols of a class in the 44 other streams / in the last channel (level 0, band x10, Cg)
# regimes with no mass 20.5 levels below a one-symbol alphabet {0}: there, and only there, that symbol owns the whole range (census, "A1")
FF_REGIMES = ("floor", "dominant", "off_hi")

_census = {}


def _census_of(name, image):
    if (name, image) not in _census:
        _census[(name, image)] = mr.census(mr.regime_images(name)[image], mr.oracle_weights(name), mr.half_levels(name))
    return _census[(name, image)]


def _need(name, image, *classes):
    c = _census_of(name, image)
    for k in classes:
        assert c["other"][k] >= MIN_OTHER and c["last"][k] >= MIN_LAST, (name, "abcd"[image], k, c)


def test_regime_table_is_finite_and_complete():
    assert set(mr.REGIME_NAMES) == {"floor", "grid", "bound_w", "dominant", "off_hi", "off_lo", "bimodal", "huge", "scales"}
    for name in mr.REGIME_NAMES + mr.B_NAMES:
        sd = mr.regime_state_dict(name)
        head = 60 if name.endswith("_b") else 88
        n = 0
        for k, v in sd.items():
            assert np.isfinite(v).all(), (name, k)
            if k.endswith("layers1toL.2.weight"):
                assert v.shape == (60, head, 1, 1)
                b = sd[k[:-6] + "bias"]
                for c, want in mr.pinned(name).items():
                    assert not v[c].any() and b[c].view(np.uint32) == np.float32(want).view(np.uint32), (name, k, c)
                    assert (np.signbit(v[c]) == np.signbit(want)).all(), (name, k, c)          # (a zero row carries its bias's sign)
                n += 1
        assert n == 3
    assert mr.half_levels("grid") == [-1, 0, 12, -31] and mr.half_levels("off_lo") == []
    # the five sigma forms of `floor`: +0, a negative number, a denormal, -0 and a normal below the floor
    s = np.asarray(mr.REGIMES["floor"]["sigma"], np.float32)
    assert s.view(np.uint32)[0] == 0 and s[1] < 0 and 0 < s[2] < np.finfo(np.float32).tiny and s.view(np.uint32)[3] == 0x80000000
    assert 0 < s[4] < np.float32(0.11) / np.float32(255)


@pytest.mark.parametrize("name", mr.REGIME_NAMES)
def test_pinned_rows_reach_the_coder(name):
    """band_params returns the pinned biases bit for bit in the pinned channels, at every position of every level and band"""
    W_o = mr.oracle_weights(name)
    planes, _ = orc.lift(mr.regime_images(name)[1])
    pins = mr.pinned(name)
    assert pins
    for lvl in range(5):
        for band in range(3):
            par = orc.band_params(planes, lvl, band, W_o).view(np.uint32)
            for c, want in pins.items():
                assert (par[..., c] == np.float32(want).view(np.uint32)).all(), (name, lvl, band, c)


@pytest.mark.parametrize("name", mr.REGIME_NAMES)
def test_oracle_round_trips_every_container(name):
    """(mr.oracle_container decodes what it encoded and compares)"""
    for image in range(4):
        sizes = {kind: sum(len(s) for row in mr.oracle_container(name, image, kind) for s in row) for kind in ("ac", "rans1", "wrans3", "xrans1", "xrans3")}
        assert all(n > 17 for n in sizes.values()), sizes


@pytest.mark.parametrize("name", mr.REGIME_NAMES)
def test_second_reader_decodes_the_xwide_containers(name):
    img, W_o = mr.regime_images(name)[0], mr.oracle_weights(name)
    for kind in ("xrans1", "xrans3"):
        segs = rr.segments(mr.oracle_container(name, 0, kind))
        planes, info = rr.decode_image(segs, rr.OraclePlanes(segs, W_o))
        assert (info["header"]["L"], info["header"]["M"]) == (256, mr.RANS_KINDS[kind][0])
        assert np.array_equal(orc.unlift(planes), img), (name, kind)


@pytest.mark.parametrize("name", mr.REGIME_NAMES)
def test_census_conditions(name):
    for image in range(4):
        print(name, "abcd"[image], _census_of(name, image))
    if name == "scales":
        c = _census_of(name, 1)                           # a spike on a pedestal: no flat stretch, not one symbol of frequency 1
        assert c["other"]["F1"] == 0 and c["last"]["F1"] == 0, c
    else:
        _need(name, 1, "F1")
    if name in ("floor", "dominant"):
        _need(name, 0, "FH")
    if name in ("off_lo", "grid"):
        _need(name, 0, "S0", "ST")
    if name == "grid":
        _need(name, 0, "Z0")
    # image (c): both chroma alphabets have ONE symbol; it owns the whole range where the regime leaves entry 0 at 0
    _need(name, 2, "A1")
    c = _census_of(name, 2)
    assert c["last"]["A1"] == c["last"]["S0"] == c["last"]["ST"] == 33 * 47, c
    if name in FF_REGIMES:
        _need(name, 2, "FF")
    if name in ("off_hi", "off_lo"):                      # the saturated case the device's container stride must hold
        img = mr.regime_images(name)[1]
        n = sum(len(s) for row in mr.oracle_container(name, 1, "ac") for s in row)
        assert n > 1.9 * img.size, (name, n, img.size)
