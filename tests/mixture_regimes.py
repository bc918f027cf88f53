"""Adversarial mixture regimes, driven from the INPUTS (numpy and the CPU oracle only; shared by tests/test_mixture_regimes_cpu.py and
tests/test_hip_mixture_regimes.py).

The decoders take their mixture parameters from the CNN, so the only way to hand them a chosen row without touching the code under test is a
model that emits it: a last 1x1 layer (`layers1toL.2`) whose weight row is zero emits its bias at every position of every band and level.
regime_state_dict(name) pins groups of the 60 outputs (sigma 0:15, mean 15:30, weight 30:45, coefficients 45:60; five components per colour,
tiled x 3) of the trained-like fixture weights that way; everything not pinned is what the base model computes ("CNN").

A pinned row is zero WITH THE SIGN OF ITS BIAS: relu leaves the hidden layer >= +0, so a +0 row adds +0 at every k of the fmaf chain and a
bias of -0.0 would arrive as +0.0 (-0 + +0 = +0 under round-to-nearest); a -0 row adds -0 and the bias arrives with every bit it has.

Finite values only: what a NaN or an Inf CNN output does is not part of numerics spec v1 and is out of scope here.

census(img, W_o) counts, from orc.lift / orc.band_params / orc.stream_pairs alone, how many symbols of an image fall into each class the
regimes exist for; tests/test_mixture_regimes_cpu.py asserts minimum counts, so a change of a fixture or of a generator that empties a class
fails there instead of silently turning the GPU test into a test of ordinary content."""
import os

import numpy as np

from helpers import bw_image, make_image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H, W = 67, 93                 # the smallest shape the suite already runs every lane kind at (xrans1 included); odd edges at every level
LAST = (0, 2, 2)              # (level, band, colour) of the last stream: level 0, band x10, Cg -- the channel the tail kernel decodes from
CLASSES = ("F1", "FH", "FF", "A1", "S0", "ST", "Z0")

_f = np.float32
_L = _f(255)


def _lv(*v):
    """grey levels -> plane units, as float32 divisions (the grid's own arithmetic: (k + 0.5) / 255 is then a sample point bit for bit)"""
    return [_f(x) / _L for x in v]


# name -> pinned groups of five (None: the CNN's own) and whether the coefficient rows are zeroed ("coef 0": the effective mean is the bias)
REGIMES = {
    # sigma at its floor, arriving as 0, a negative number, a denormal, -0.0 and a small normal: max(sigma, 0.11 / 255) on every one.  The base
    # model's weights are within 0.001 of their biases and no Cg component of band x10 has a share above 0.32, so five spikes never give
    # that channel a symbol of half the range: "wboost" adds 6 to the BIAS of component 0's weight channels (rows untouched: still the CNN's
    # output, share 0.74) -- without it the last channel of image (a) held 0 .. 6 such symbols over 40 seeds, with it about 1,000.
    "floor":    dict(sigma=[0.0, -1.0, 1e-40, -0.0, 1e-4], wboost=[6.0, 0.0, 0.0, 0.0, 0.0]),
    # means ON sample points ((k + 0.5) / 255: k = -1, 0, 12, -31; the fifth on an integer) under sigmas at and near the floor: erfc_spec(+-0)
    "grid":     dict(sigma=_lv(0.11, 0.2, 0.3, 0.11, 0.25), mean=_lv(-0.5, 0.5, 12.5, -30.5, 100.0), coef0=True),
    # every weight at or below its 1e-6 bound: the sum is 5e-6 and the 1e-9f of the denominator is 2e-4 of it
    "bound_w":  dict(sigma=_lv(8, 8, 8, 8, 8), weight=[0.0, -1.0, 1e-6, 1e-7, 0.0]),
    # one narrow component that owns nearly everything, in front of four wide ones at the weight bound: a symbol above half the range
    "dominant": dict(sigma=_lv(0.6, 30, 30, 30, 30), weight=[100.0, 1e-7, -3.0, 1e-6, 1e-6]),
    # the whole mixture above / below the value range: a saturated CDF, every symbol of frequency 1 (2 bytes each).  off_hi: 1,275 levels above,
    # every entry i is i.  off_lo: 132.6 levels below zero with sigma 8 -- a chroma alphabet that starts above -100 (images (a), (c)) has all its
    # entries at the top (entry 0 = 65536 - (Lp - 1): the floor of the search is NOT 0), one that starts at -255 (images (b), (d)) is flat at 0
    # below the step and flat at 1 above it, and Y (min -127) has entry 0 = 2,041, a bottom symbol of frequency 48,690, a tail of 25 symbols
    # and the saturated stretch behind it.  With the mean at -5.0 every table is saturated whatever the seed, and image (a) -- an arithmetic
    # decoder fed bytes no encoder of such tables writes -- never had more than 11 bottom symbols in its last channel over 400 seeds.
    "off_hi":   dict(sigma=_lv(2, 2, 2, 2, 2), mean=[5.0] * 5, coef0=True),
    "off_lo":   dict(sigma=_lv(8, 8, 8, 8, 8), mean=[-0.52] * 5, coef0=True),
    # two narrow modes 120 levels apart, a flat gap around the median between them
    "bimodal":  dict(sigma=_lv(0.5, 0.5, 0.5, 0.5, 0.5), mean=_lv(-60, 60, 0, 0, 0), weight=[1.0, 1.0, 0.0, 0.0, 0.0], coef0=True),
    # sigmas of 255,000 levels: a CDF that is a straight line through 1/2
    "huge":     dict(sigma=[1000.0] * 5),
    # five scales at once, equal weights: a spike on a pedestal, no flat stretch anywhere
    "scales":   dict(sigma=[0.0] + _lv(1, 30) + [3.0, 1e3], weight=[1.0] * 5),
}
B_TWINS = ("grid", "off_lo")                      # regimes that also exist on config B (60-wide heads, 2 levels): names "<regime>_b"
REGIME_NAMES = tuple(REGIMES)
B_NAMES = tuple(r + "_b" for r in B_TWINS)
SEEDS = {"grid": 1, "off_lo": 9}                  # regime -> seed of the random bytes image (a) is decoded from (default 5): chosen for the census
GROUPS = (("sigma", 0), ("mean", 15), ("weight", 30))


def _split(name):
    return (name[:-2], True) if name.endswith("_b") else (name, False)


def pinned(name):
    """{output channel: float32 bias} of the regime: what band_params must return, bit for bit, in those channels at every position"""
    reg = REGIMES[_split(name)[0]]
    out = {}
    for key, c0 in GROUPS:
        if reg.get(key) is not None:
            five = np.asarray(reg[key], dtype=np.float32)
            assert five.shape == (5,) and np.isfinite(five).all()
            for c in range(15):
                out[c0 + c] = five[c % 5]
    if reg.get("coef0"):
        for c in range(45, 60):
            out[c] = _f(0.0)
    return out


def regime_state_dict(name):
    """The trained-like fixture weights (config B's for a "<regime>_b" name) with the regime's groups pinned in every band's last layer."""
    base, is_b = _split(name)
    sd = {k: np.array(v) for k, v in np.load(os.path.join(GOLDEN, "weights_b_trainedlike.npz" if is_b else "weights_trainedlike.npz")).items()}
    pins = pinned(name)
    nband = 0
    for k in sd:
        if k.endswith("layers1toL.2.bias"):
            wk = k[:-4] + "weight"
            b, w = sd[k].astype(np.float32), sd[wk].astype(np.float32)
            assert b.shape == (60,) and w.shape[0] == 60
            for c, v in pins.items():
                b[c] = v
                w[c] = np.copysign(_f(0.0), v)
            if REGIMES[base].get("wboost") is not None:
                b[30:45] += np.tile(np.asarray(REGIMES[base]["wboost"], dtype=np.float32), 3)
            sd[k], sd[wk] = b, w
            nband += 1
    assert nband == 3
    return sd


_weights = {}


def oracle_weights(name):
    """orc.Weights of a config-A regime (the oracle restates config A only), cached"""
    from llicti_amd.weights import pack_state_dict
    from oracle import oracle as orc
    assert not _split(name)[1]
    if name not in _weights:
        _weights[name] = orc.Weights(pack_state_dict(regime_state_dict(name)))
    return _weights[name]


def grey_image(seed=13):
    """grey noise, R = G = B: Co = Cg = 0 everywhere, so both chroma alphabets have ONE symbol (Lp = 2)"""
    g = np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)
    return np.stack([g, g, g])


_images = {}


def regime_images(name):
    """[(a) drawn from the regime's own model, (b) i.i.d. noise, (c) grey noise, (d) black / white (Lp = 512)], each 67 x 93.  (a) is
    helpers.make_sampled_image's method under the regime's weights: the oracle's reference-format decoder fed seeded random bytes behind the
    header of the smooth image.  A config-B twin gets the images of its config-A regime (the oracle cannot draw from a config-B model)."""
    from oracle import oracle as orc
    name = _split(name)[0]
    if name not in _images:
        W_o = oracle_weights(name)
        bl = orc.encode_image(make_image("smooth", H, W, 11), W_o)
        rng = np.random.default_rng(SEEDS.get(name, 5))
        bl = [list(bl[0])] + [[rng.integers(0, 256, len(s), dtype=np.uint8).tobytes() for s in row] for row in bl[1:]]
        imgs = [orc.decode_image(bl, W_o), make_image("noise", H, W, 3), grey_image(), bw_image(H, W)]
        for im in imgs:
            im.setflags(write=False)
        _images[name] = imgs
    return _images[name]


def half_levels(name):
    """the k of the regime's pinned means that are (k + 0.5) / 255 bit for bit"""
    mean = REGIMES[_split(name)[0]].get("mean")
    out = []
    for m in ([] if mean is None else mean):
        k = int(np.floor(float(m) * 255.0))
        if abs(k) <= 300 and _f(k + 0.5) / _L == _f(m):
            out.append(k)
    return out


def census(img, W_o, half=()):
    """{"last" | "other": {class: symbols}} of one image under one model: "last" is the stream of LAST, "other" the 44 others.
      F1  frequency 1                         FH  frequency >= 0x8000             FF  frequency 0x10000 (the whole range)
      S0  the bottom symbol                   ST  the top symbol (c_high = 0x10000, stored as 0 in 16 bits)
      A1  the only symbol of its alphabet (Lp = 2): bottom and top at once.  Its c_low is entry 0 = rint(cdf((min - 20.5) / 255) * 65535), so it
          is an FF symbol only under a mixture with no mass 20.5 levels below it; under off_lo it has frequency 1 and costs 16 bits.
      Z0  (half = the k of pinned means (k + 0.5) / 255, coefficients zero) plane value k below the top symbol or k + 1 above the bottom one:
          the symbol's upper / lower table entry samples the mean itself and evaluates erfc_spec(+-0)."""
    from oracle import oracle as orc
    planes, mm = orc.lift(img)
    out = {"last": dict.fromkeys(CLASSES, 0), "other": dict.fromkeys(CLASSES, 0)}
    for lvl in range(5):
        for band in range(3):
            par = orc.band_params(planes, lvl, band, W_o)
            for clr in range(3):
                lo, hi, sym = orc.stream_pairs(planes, mm, lvl, band, clr, par)
                lo, hi, sym = lo.astype(np.int64), hi.astype(np.int64), sym.astype(np.int64)
                minv = -127 if clr == 0 else int(mm[clr])
                maxv = 128 if clr == 0 else int(mm[3 + clr])
                f, v = hi - lo, sym + minv
                assert (f >= 1).all() and (hi <= 0x10000).all() and ((hi == 0x10000) == (sym == maxv - minv)).all()
                z = np.zeros(sym.shape, bool)
                for k in half:
                    z |= ((v == k) & (v < maxv)) | ((v == k + 1) & (v > minv))
                d = out["last" if (lvl, band, clr) == LAST else "other"]
                for key, m in (("F1", f == 1), ("FH", f >= 0x8000), ("FF", f == 0x10000), ("A1", (sym == 0) & (hi == 0x10000)), ("S0", sym == 0),
                               ("ST", hi == 0x10000), ("Z0", z)):
                    d[key] += int(m.sum())
    return out


# (streams, lane kind) of the rANS containers the tests code, by the codec's name for them
RANS_KINDS = {"rans1": (1, 0), "rans4": (4, 0), "wrans3": (3, 1), "xrans1": (1, 2), "xrans3": (3, 2)}
_containers = {}


def oracle_container(name, image, kind):
    """The oracle's bytestream_list of image `image` (0 .. 3) of a config-A regime: kind "ac" (the reference format) or a key of RANS_KINDS.
    Computed once per process and checked on the spot: the oracle decodes it back to the image."""
    from oracle import oracle as orc
    key = (name, image, kind)
    if key not in _containers:
        img, W_o = regime_images(name)[image], oracle_weights(name)
        if kind == "ac":
            bl = orc.encode_image(img, W_o)
            back = orc.decode_image(bl, W_o)
        else:
            bl = orc.encode_image_rans(img, W_o, *RANS_KINDS[kind])
            back = orc.decode_image_rans(bl, W_o)
        assert np.array_equal(back, img), key
        _containers[key] = bl
    return _containers[key]
