"""The CPU oracle against a float64 restatement of the model (tests/ref64.py), on the tile-edge sweep shapes (helpers.SWEEP_SHAPES), with
rigorous per-output bounds; deliberately wrong variants of the float64 reference must break those bounds (so the bounds are tight enough to
catch a subtle error); erfc_spec's error budget; and the plan's workspace for a call that mixes fixed and "auto" xwide stream counts.  CPU only."""
import numpy as np
import pytest

import ref64
from conftest import load_state_dict
from helpers import SWEEP_SHAPES, all_tile_edge_classes, make_image, tile_edge_classes

WEIGHTS = ("trainedlike", "rand1337")
NOISE_SHAPES = {("rand1337", (67, 196)), ("rand1337", (70, 133))}     # full-range Co / Cg alphabets (Lp ~ 512): the costly table checks


def _image(wname, H, W):
    kind = "noise" if (wname, (H, W)) in NOISE_SHAPES else "smooth"
    return make_image(kind, H, W, seed=H * 1000 + W)


class _Case:
    """One sweep image: planes, fp32 float planes, the oracle's CNN outputs per (level, band)."""

    def __init__(self, wname, H, W):
        from llicti_amd.weights import pack_state_dict
        from oracle import oracle as orc
        self.sd = load_state_dict(wname)
        self.W_o = orc.Weights(pack_state_dict(self.sd))
        self.rgb = _image(wname, H, W)
        self.planes, self.mm = orc.lift(self.rgb)
        self.fp = self.planes.astype(np.float32) / np.float32(255)
        self.H, self.W = H, W
        self.par = {(lvl, band): orc.band_params(self.planes, lvl, band, self.W_o) for lvl in range(5) for band in range(3)}

    def stage(self, lvl, band):
        """-> coded positions' CNN outputs [n, 60] and targets / 255 (fp32) [3, n] of a stage (the band's cropped positions)."""
        a, b = ref64.TARGET[band]
        rows = np.arange(a << lvl, self.H, 2 << lvl)
        cols = np.arange(b << lvl, self.W, 2 << lvl)
        P = self.par[(lvl, band)][:len(rows), :len(cols)].reshape(-1, 60)
        tg = self.planes[:, rows][:, :, cols].reshape(3, -1).astype(np.float32) / np.float32(255)
        return P, tg

    def alphabet(self, clr):
        return (-127, 128) if clr == 0 else (int(self.mm[clr]), int(self.mm[3 + clr]))


_cases = {}


def case(wname, H, W):
    if (wname, H, W) not in _cases:
        _cases[(wname, H, W)] = _Case(wname, H, W)
    return _cases[(wname, H, W)]


def test_sweep_covers_every_tile_edge_class():
    got = set()
    for H, W in SWEEP_SHAPES:
        got |= tile_edge_classes(H, W)
    assert len(all_tile_edge_classes()) == 72
    assert got == all_tile_edge_classes(), sorted(all_tile_edge_classes() - got)


@pytest.mark.parametrize("wname", WEIGHTS)
def test_oracle_cnn_within_float64_bound(wname):
    """orc.band_params within cnn_error_bound of band_params64 at every level, band, position and output of every sweep shape, and at the
    coarse levels of the two extreme aspect ratios."""
    from oracle import oracle as orc
    worst = 0.0
    for H, W in SWEEP_SHAPES:
        c = case(wname, H, W)
        for lvl in range(5):
            for band in range(3):
                ref = ref64.band_params64(c.fp, lvl, band, c.sd)
                bnd = ref64.cnn_error_bound(c.fp, lvl, band, c.sd)
                got = c.par[(lvl, band)]
                assert got.shape == ref.shape
                r = (np.abs(got - ref) / bnd).max()
                assert r <= 1.0, (H, W, lvl, band, r)
                worst = max(worst, r)
    c = case(wname, 67, 133)
    for H, W in ((8160, 32), (32, 8160)):
        rgb = make_image("noise", H, W, seed=H + W)
        planes, _ = orc.lift(rgb)
        fp = planes.astype(np.float32) / np.float32(255)
        for lvl in (2, 3, 4):
            for band in range(3):
                got = orc.band_params(planes, lvl, band, c.W_o)
                r = (np.abs(got - ref64.band_params64(fp, lvl, band, c.sd)) / ref64.cnn_error_bound(fp, lvl, band, c.sd)).max()
                assert r <= 1.0, (H, W, lvl, band, r)
                worst = max(worst, r)
    print(f"{wname}: largest |oracle - float64| / bound of the CNN outputs: {worst:.3g}")


@pytest.mark.parametrize("wname", WEIGHTS)
def test_oracle_tables_within_float64_tolerance(wname):
    """Every entry of every table row of every stage (level, band, colour) of every sweep shape: orc.cdf_rows within cdf_tolerance of the
    float64 mixture CDF."""
    from oracle import oracle as orc
    worst = 0.0
    for H, W in SWEEP_SHAPES:
        c = case(wname, H, W)
        for lvl in range(5):
            for band in range(3):
                P, tg = c.stage(lvl, band)
                for clr in range(3):
                    minv, maxv = c.alphabet(clr)
                    got = orc.cdf_rows(P, clr, tg[0], tg[1], minv, maxv)
                    ent, tol = ref64.cdf_entries64(P, clr, tg[0], tg[1], minv, maxv)
                    r = (np.abs(ref64.wrap_diff(got, ent)) / tol).max()
                    assert r <= 1.0, (H, W, lvl, band, clr, r)
                    worst = max(worst, r)
    print(f"{wname}: largest |oracle - float64| / tolerance of the table entries: {worst:.3g}")


@pytest.mark.parametrize("wname", WEIGHTS)
def test_oracle_selfinfo_within_float64_tolerance(wname):
    from oracle import oracle as orc
    worst = 0.0
    for H, W in SWEEP_SHAPES[::3]:
        c = case(wname, H, W)
        fp = orc.lift_train(c.rgb)
        for lvl in range(5):
            for band in range(3):
                par = orc.band_params_f(fp, lvl, band, c.W_o)
                got = orc.selfinfo(fp, lvl, band, par)
                ref, tol = ref64.selfinfo64(fp, lvl, band, par)
                r = (np.abs(got - ref) / tol).max()
                assert r <= 1.0, (H, W, lvl, band, r)
                worst = max(worst, r)
    print(f"{wname}: largest |oracle - float64| / tolerance of the self-information: {worst:.3g}")


@pytest.mark.parametrize("mutant", ref64.MUTANTS)
def test_float64_mutants_break_their_bounds(mutant):
    """A wrong float64 reference must be caught by the same comparison: the bounds are tight enough to see a one-row / one-column geometry
    error, a dropped term of the mean update and the grid's end points."""
    from oracle import oracle as orc
    for wname in WEIGHTS:
        for H, W in SWEEP_SHAPES:
            c = case(wname, H, W)
            for lvl in range(5):
                for band in range(3):
                    if mutant in ("no_odd_pad", "tap_shift"):
                        ref = ref64.band_params64(c.fp, lvl, band, c.sd, mutant=mutant)
                        bnd = ref64.cnn_error_bound(c.fp, lvl, band, c.sd)
                        if (np.abs(c.par[(lvl, band)] - ref) > bnd).any():
                            return
                        continue
                    P, tg = c.stage(lvl, band)
                    for clr in ((2,) if mutant == "cg_no_co" else (0, 1, 2)):
                        minv, maxv = c.alphabet(clr)
                        got = orc.cdf_rows(P, clr, tg[0], tg[1], minv, maxv)
                        _, tol = ref64.cdf_entries64(P, clr, tg[0], tg[1], minv, maxv)
                        bad, _ = ref64.cdf_entries64(P, clr, tg[0], tg[1], minv, maxv, mutant=mutant, with_tolerance=False)
                        if (np.abs(ref64.wrap_diff(got, bad)) > tol).any():
                            return
    pytest.fail(f"mutant {mutant!r} of the float64 reference stays within every bound on the sweep")


def test_erfc_spec_error_budget():
    """erfc_spec (the oracle's) against float64 erfc on a sample: |err| <= ERFC_REL erfc(|x|) + erfc(7) (it is 0 from 7 on), + u for x < 0
    (the rounding of 2 - v) -- the budget ref64's tolerances assume.  The sample is kept as a quick check; the claim itself is held for every
    fp32 input by tests/test_numerics_cpu.py::test_erfc_budget_holds_for_every_float, and numerics.hpp's erfc_spec is held to the oracle's bits
    on every input by tests/test_hip_numerics.py.  Exhaustive maxima (tests/golden/numerics_sums.npz): 3.5577e-7 = 5.97 u relative on [0, 7),
    at x = 2.0307915 (0x4001f87d); 3.25006e-7 absolute below 0, at x = -0.039951678 (0xbd23a45f); error / budget at most 1 / (1 + 6 u), at
    x = 7 where erfc_spec drops to 0.  ERFC_REL was 5 u on the strength of this sample (2.74e-7 = 4.6 u); the sweep made it 6 u."""
    import math
    from oracle import oracle as orc
    rng = np.random.default_rng(5)
    xs = [np.linspace(-7.5, 7.5, 200_001, dtype=np.float32), rng.uniform(-7.5, 7.5, 20_000).astype(np.float32)]
    edges = []
    for e in range(-30, 3):                                          # binade edges of |x| (and their neighbours)
        for v in (2.0 ** e, 1.5 * 2.0 ** e):
            if v <= 7.5:
                f = np.float32(v)
                edges += [np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(8))]
    edges = np.array(edges, np.float32)
    near = np.concatenate([np.float32(7.0) + np.arange(-200, 201, dtype=np.float32) * np.float32(2 ** -21),
                           np.arange(-200, 201, dtype=np.float32) * np.float32(2 ** -30), [0.0, -0.0]]).astype(np.float32)
    x = np.concatenate(xs + [edges, -edges, near, -near]).astype(np.float32)
    got = orc.erfc(x).astype(np.float64)
    ref = np.array([math.erfc(float(v)) for v in x])
    refa = np.array([math.erfc(abs(float(v))) for v in x])
    budget = ref64.ERFC_REL * refa + ref64.ERFC_TAIL + ref64.U * (x < 0)
    err = np.abs(got - ref)
    bad = err > budget
    assert not bad.any(), (x[bad][:5], err[bad][:5], budget[bad][:5])
    pos = (x >= 0) & (x < 7)
    print(f"erfc_spec: largest relative error on [0, 7): {(err[pos] / refa[pos]).max():.3g}; largest absolute below 0: {err[x < 0].max():.3g}")


@pytest.mark.parametrize("sizes", [[(2160, 3840), (512, 768)], [(512, 768), (2160, 3840)], [(2160, 3840), (512, 768), (2160, 3840)]])
def test_workspace_mixed_fixed_and_auto_xwide(sizes):
    """Container "auto" with one image of >= 4.3 MP beside smaller ones: the large image's count is a fixed 64 xwide streams, the others' an
    encoder-picked ("auto") count.  The call must be accepted (workspace > 0) with every image in its own mode, and its workspace must cover
    each image's own."""
    import ctypes as C
    from llicti_amd import _lib
    from llicti_amd.codec import auto_modes, image_mode
    modes = auto_modes(sizes)
    mixed = len(set(sizes)) > 1
    assert modes == [image_mode(h, w, mixed) for h, w in sizes]
    assert len({m & 0x10000 for m in modes}) == 2                   # (fixed and auto in one call)
    L = _lib.lib()
    B = len(sizes)
    Hs = (C.c_int * B)(*[h for h, _ in sizes])
    Ws = (C.c_int * B)(*[w for _, w in sizes])
    md = (C.c_int * B)(*modes)
    total = L.llicti_workspace_bytes_vm(B, Hs, Ws, md)
    assert total > 0, _lib.lib().llicti_last_error()
    for (h, w), m in zip(sizes, modes):
        one = L.llicti_workspace_bytes_vm(1, (C.c_int * 1)(h), (C.c_int * 1)(w), (C.c_int * 1)(m))
        assert 0 < one <= total
