"""The CPU oracle's erfc_spec over every fp32 input, through tests/golden/numerics_sums.npz (tests/golden/make_numerics_sums.py; the host
program is tests/numerics_sums_host.c): a guard that recomputes a fixed subset of the fixture, the float64 error budget of tests/ref64.py
as a condition on all 2^32 inputs, and the saturation facts cdf_table_kernel's constant fill relies on.  CPU only; the device side of the
same sweep is tests/test_hip_numerics.py."""
import time

import numpy as np
import pytest

import numerics_sums as ns
import ref64

ONE, TWO = 0x3F800000, 0x40000000               # bits of 1.0f, 2.0f


@pytest.fixture(scope="module")
def fx():
    return np.load(ns.FIXTURE)


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return ns.build_host(tmp_path_factory.mktemp("numerics_sums"))


def test_fixture_guard(fx, host_exe):
    """The committed fixture is what the current oracle gives: the two sums, the extreme words and the reciprocal sums of 32 chunks (16 of a
    seeded draw, those around +-0, 1, +-7, +-inf, the NaNs) recomputed and compared; the oracle's source hash and the budget constants the
    ratios were taken against are the current ones.  An oracle or ERFC_REL edit therefore forces tests/golden/make_numerics_sums.py to be
    run again.  The error maxima depend on libm's float64 erfc: a libm that rounds it differently (1 ulp of float64 in the reference is
    2^-53 / 3e-7 = 4e-10 of an error this size) must still agree to 1e-6.  Measured: 1.1 s for the 32 chunks with 8 threads on 8 CPUs (the test prints it), the build of the host program besides."""
    assert str(fx["oracle_sha256"]) == ns.oracle_sha256(), "oracle/ changed: rerun tests/golden/make_numerics_sums.py"
    assert float(fx["budget_rel"]) == ref64.ERFC_REL and float(fx["budget_tail"]) == ref64.ERFC_TAIL, "ERFC_REL / ERFC_TAIL changed: regenerate"
    assert int(fx["recip_chunk0"]) == ns.RECIP_CHUNK0 and fx["recip_s1"].shape == (ns.RECIP_NCHUNKS,)
    cs = ns.guard_chunks()
    assert len(cs) == 32
    t0 = time.time()
    r = ns.run_host(host_exe, ["chunks"] + [str(c) for c in cs], timeout=600)
    print(f"host subset of {len(cs)} chunks: {time.time() - t0:.2f} s")
    assert list(r["chunk"]) == cs
    for got, name in (("s1", "erfc_s1"), ("s2", "erfc_s2"), ("min", "erfc_min"), ("max", "erfc_max")):
        bad = np.flatnonzero(r[got] != fx[name][cs])
        assert bad.size == 0, (name, [cs[i] for i in bad[:5]])
    for got, name in (("rel", "rel_max"), ("abs", "abs_max"), ("ratio", "ratio_max")):
        assert np.allclose(r[got], fx[name][cs], rtol=1e-6, atol=0.0), name
    in_range = [c for c in cs if ns.RECIP_CHUNK0 <= c < ns.RECIP_CHUNK0 + ns.RECIP_NCHUNKS]
    assert sorted(r["recip"]) == in_range and len(in_range) >= 2
    for c in in_range:
        i = c - ns.RECIP_CHUNK0
        assert r["recip"][c] == (int(fx["recip_s1"][i]), int(fx["recip_s2"][i])), c


def test_erfc_budget_holds_for_every_float(fx):
    """|erfc_spec(x) - erfc(x)| <= ERFC_REL erfc(|x|) + ERFC_TAIL + u [x < 0] for EVERY fp32 x that is not a NaN: the assumption under every
    tolerance of tests/ref64.py, as a condition on the exhaustive sweep and not a measurement of it.  (With ERFC_REL = 5 u, which a sample of
    220 thousand points had supported, the largest ratio is 1.19, at x = 2.0307915: hence 6 u.)"""
    i, j, k = int(fx["rel_max"].argmax()), int(fx["abs_max"].argmax()), int(fx["ratio_max"].argmax())
    print(f"largest relative error on [0, 7): {fx['rel_max'][i]:.6g} = {fx['rel_max'][i] / ref64.U:.3f} u at x = {ns.bits_to_float(fx['rel_arg'][i])!r}; "
          f"largest absolute error below 0: {fx['abs_max'][j]:.6g} at x = {ns.bits_to_float(fx['abs_arg'][j])!r}; "
          f"largest error / budget: {fx['ratio_max'][k]!r} at x = {ns.bits_to_float(fx['ratio_arg'][k])!r}")
    assert fx["ratio_max"].shape == (ns.NCHUNKS,)
    assert fx["ratio_max"][k] <= 1.0, (float(fx["ratio_max"][k]), hex(int(fx["ratio_arg"][k])))
    # ERFC_REL is the measured maximum rounded up to a whole multiple of u, not a looser figure
    assert ref64.ERFC_REL / ref64.U == np.ceil(fx["rel_max"][i] / ref64.U)


def test_erfc_saturation_facts(fx, host_exe, tmp_path):
    """What cdf_table_kernel's constant fill assumes of erfc_spec (cdf.hpp: a component whose argument has |x| >= 7 contributes exactly 0 or
    wn): 0 for every x >= 7, +inf and every NaN of either sign; 2 for every x <= -7 and -inf; 1 at +0 and -0; and not yet 0 just below 7.
    Whole chunks are read off the fixture's extreme words, the chunks with a boundary inside off the host program's dumps."""
    lo7, hi7 = 0x40E00000 >> ns.CHUNK_BITS, 0xC0E00000 >> ns.CHUNK_BITS          # 7.0f and -7.0f are the first words of their chunks
    assert (0x40E00000 & (ns.CHUNK - 1)) == 0 and (0xC0E00000 & (ns.CHUNK - 1)) == 0
    mn, mx = fx["erfc_min"], fx["erfc_max"]
    assert (mx[lo7:0x800] == 0).all()                              # [7, +inf], the positive NaNs
    assert (mn[hi7:0xFF8] == TWO).all() and (mx[hi7:0xFF8] == TWO).all()          # [-7, -inf)
    assert (mx[0xFF9:] == 0).all()                                 # negative NaNs
    assert mn[lo7 - 1] > 0                                         # the chunk below 7: still positive
    inf_neg = ns.host_dump(host_exe, 0xFF8, tmp_path / "ff8.bin")  # -inf, then negative NaNs
    assert inf_neg[0] == TWO and (inf_neg[1:] == 0).all()
    zero_pos = ns.host_dump(host_exe, 0x000, tmp_path / "000.bin")
    zero_neg = ns.host_dump(host_exe, 0x800, tmp_path / "800.bin")
    assert zero_pos[0] == ONE and zero_neg[0] == ONE
    # the dumps are the words the sums were taken of
    k = np.arange(ns.CHUNK, dtype=np.uint64)
    for c, w in ((0xFF8, inf_neg), (0x000, zero_pos), (0x800, zero_neg)):
        w64 = w.astype(np.uint64)
        assert int(w64.sum()) == int(fx["erfc_s1"][c]) and int(((2 * k + 1) * w64).sum()) == int(fx["erfc_s2"][c]), c
