"""Resized crops, the parts that need no GPU: the weight rule the kernel is compiled from (llicti_resize_axis) against tests/ref_resize.py bit for
bit, llicti_resize_window_ok against plain inequalities, codec.resized_crop_plan, the arithmetic spec against torch's F.interpolate on the CPU,
and the host validation (resolve_resize) compiled by g++ into a stand-alone driver."""
import ctypes as C
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch

import ref_resize as rr
from llicti_amd import _lib
from llicti_amd import codec as cd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ["llicti_resize_window_ok", "llicti_resize_axis", "llicti_decode_images_tensor_resized"]


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "llicti_hip.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and re.search(r"\b%s\(" % name, header), name
        decl = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(decl.split(",")) == len(_lib._SIGS[name][1]) == len(getattr(L, name).argtypes), name
    assert cd.RESIZE_TAP_MAX == rr.TAP_MAX == 9


# ------------------------------------------------------------------------------------------------ the weight rule
NS = (1, 2, 31, 32, 33, 224, 8160)
MS = (1, 7, 224, 8160)


def _indices(m):
    if m <= 224:
        return np.arange(m)
    rng = np.random.default_rng(m)
    return np.unique(np.concatenate([[0, 1, m // 2, m - 2, m - 1], rng.integers(0, m, 40)]))


@pytest.mark.parametrize("antialias", [0, 1])
def test_weight_rule_is_the_reference_bit_for_bit(antialias):
    """llicti_resize_axis -- the host's compile of the LLICTI_HD function the kernel calls -- against ref_resize.axis_taps: the first source index,
    the tap count and every weight's 32 bits, for n in NS, m in MS (every index of a small m; first, last and random ones of a large m).
    Every total is above zero.  Wherever the call admits the pair (no filter, or n <= 4 m) the count stays within the kernel's compile-time
    bound and the weights sum to 1 within 2 ulp.  The pairs the call refuses (the filter on at a scale above 4: up to 8160 taps) are held to
    the reference's bits all the same, but not to those two properties: they are what the refusal exists for -- 8160 taps are above any bound,
    and a sum of thousands of separately rounded quotients is not within 2 ulp of 1 under the arithmetic the header fixes (the reference,
    bit-equal, shows the same 5.6e-7 at 8160 -> 7)."""
    L = _lib.lib()
    n_idx = 0
    for n, m in itertools.product(NS, MS):
        idx = _indices(m)
        lo, cnt, w, total = rr.axis_taps(n, m, antialias, idx)
        assert (total > 0).all(), (n, m)
        assert (cnt >= 1).all() and (lo >= 0).all() and (lo + cnt <= n).all(), (n, m)
        admitted = (not antialias) or n <= 4 * m
        if admitted:
            assert cnt.max() <= rr.TAP_MAX, (n, m, int(cnt.max()))
        cap = max(int(cnt.max()), rr.TAP_MAX) + 1
        buf = np.empty(cap, dtype=np.float32)
        for row, i in enumerate(idx):
            got_lo = C.c_int(-1)
            buf.fill(np.nan)
            got = L.llicti_resize_axis(n, m, antialias, int(i), C.byref(got_lo), buf.ctypes.data_as(C.POINTER(C.c_float)), cap)
            assert (got, got_lo.value) == (int(cnt[row]), int(lo[row])), (n, m, int(i))
            want = np.zeros(cap, dtype=np.float32)
            want[:w.shape[1]] = w[row]
            assert np.array_equal(buf.view(np.uint32), want.view(np.uint32)), (n, m, int(i), buf[:got], want[:got])
            if admitted:
                assert abs(float(buf.astype(np.float64).sum()) - 1.0) <= 2 * 2.0 ** -23, (n, m, int(i))
            n_idx += 1
    assert n_idx > 1800                 # (the grid did not collapse)
    # the wrapper, a cut tap list (the weights stay those of the full sum), and arguments outside the domain
    cnt, lo, w = cd.resize_axis(96, 24, True, 5)
    assert cnt == 8 and lo == 18 and w.shape == (9,) and w[8] == 0 and abs(float(w.sum()) - 1) < 1e-6
    cnt2, lo2, w2 = cd.resize_axis(96, 24, True, 5, cap=3)
    assert (cnt2, lo2) == (cnt, lo) and np.array_equal(w2, w[:3])
    lo_c = C.c_int(0)
    for bad in ((0, 4, 1, 0), (4, 0, 1, 0), (4, 4, 1, -1), (4, 4, 1, 4)):
        assert L.llicti_resize_axis(*bad, C.byref(lo_c), buf.ctypes.data_as(C.POINTER(C.c_float)), 4) == 0, bad


def test_identity_weights_are_one_and_zero():
    """n == m: tap 0 of index i is source pixel i with weight exactly 1, the second tap (inside the box) exactly 0: a box of Ho x Wo reproduces pixels"""
    for n in (1, 2, 33, 224, 8160):
        for aa in (0, 1):
            lo, cnt, w, _ = rr.axis_taps(n, n, aa)
            assert np.array_equal(lo, np.arange(n)) and (w[:, 0] == 1).all() and (w[:, 1:] == 0).all() and cnt.max() <= 2


# ------------------------------------------------------------------------------------------------ the window check
def _window_ok(H, W, r, y0, x0, hs, ws, Ho, Wo, aa):
    if H < 1 or W < 1 or not 0 <= r <= 5:
        return False
    Hr, Wr = -(-H // (1 << r)), -(-W // (1 << r))
    ok = hs >= 1 and ws >= 1 and y0 >= 0 and x0 >= 0 and y0 + hs <= Hr and x0 + ws <= Wr and 1 <= Ho <= 8160 and 1 <= Wo <= 8160 and aa in (0, 1)
    return bool(ok and (not aa or (hs <= 4 * Ho and ws <= 4 * Wo)))


def test_resize_window_ok_against_plain_inequalities():
    L = _lib.lib()
    n = 0
    for (H, W), r in itertools.product(((32, 32), (33, 35), (67, 93), (64, 96), (512, 768), (8160, 8160)), range(6)):
        Hr, Wr = cd.reduced_dims(H, W, r)
        for (hs, ws), (Ho, Wo) in itertools.product({(1, 1), (Hr, Wr), (Hr, 1), (1, Wr), (max(1, Hr // 2), max(1, Wr // 3)), (Hr + 1, Wr), (Hr, Wr + 1), (0, 1), (1, -1)},
                                                    ((1, 1), (16, 24), (max(1, Hr // 4), max(1, Wr // 4)), (8160, 8160), (8161, 4), (4, 0))):
            for y0, x0 in itertools.product({0, Hr - hs, Hr - hs + 1, -1}, {0, 1, Wr - ws, Wr - ws + 1}):
                for aa in (0, 1):
                    want = _window_ok(H, W, r, y0, x0, hs, ws, Ho, Wo, aa)
                    assert L.llicti_resize_window_ok(H, W, r, y0, x0, hs, ws, Ho, Wo, aa) == int(want), (H, W, r, y0, x0, hs, ws, Ho, Wo, aa)
                    n += 1
    assert n > 20000
    # the scale-4 edge by name: exactly 4.0 is taken, 4 Ho + 1 rows are refused with the filter and taken without
    assert L.llicti_resize_window_ok(64, 96, 0, 0, 0, 64, 96, 16, 24, 1) == 1
    assert L.llicti_resize_window_ok(67, 96, 0, 0, 0, 65, 96, 16, 24, 1) == 0 and L.llicti_resize_window_ok(67, 96, 0, 0, 0, 65, 96, 16, 24, 0) == 1
    assert L.llicti_resize_window_ok(64, 99, 0, 0, 1, 64, 97, 16, 24, 1) == 0 and L.llicti_resize_window_ok(64, 99, 0, 0, 1, 64, 97, 16, 24, 0) == 1
    assert cd.resize_window_ok(64, 96, 0, 0, 0, 64, 96, 16, 24) is True and cd.resize_window_ok(67, 96, 0, 0, 0, 65, 96, 16, 24) is False
    for bad in ((32, 32, 0, 0, 0, 8, 8, 8, 8, 2), (32, 32, 0, 0, 0, 8, 8, 8, 8, -1), (32, 32, 6, 0, 0, 1, 1, 1, 1, 0), (0, 32, 0, 0, 0, 1, 1, 1, 1, 0),
                (32, 32, 0, 2 ** 31 - 1, 0, 2, 2, 2, 2, 0), (32, 32, 0, 0, 0, 2 ** 31 - 1, 2, 8160, 8160, 1)):
        assert L.llicti_resize_window_ok(*bad) == 0, bad


# ------------------------------------------------------------------------------------------------ resized_crop_plan
def test_resized_crop_plan():
    plan = cd.resized_crop_plan
    # full-image boxes: the largest r at which the decimated image still has the output's pixels
    assert plan([(2160, 3840)], [(0, 0, 2160, 3840)], (224, 224)) == (3, [(0, 0, 270, 480)])
    assert plan([(512, 768)], [(0, 0, 512, 768)], (224, 224)) == (1, [(0, 0, 256, 384)])
    assert plan([(8160, 8160)], [(0, 0, 8160, 8160)], (224, 224)) == (5, [(0, 0, 255, 255)])
    assert plan([(8160, 8160)], [(0, 0, 8160, 8160)], (224, 224), nlevels=2) == (2, [(0, 0, 2040, 2040)])
    assert plan([(67, 93)], [(0, 0, 67, 93)], (17, 24)) == (2, [(0, 0, 17, 24)])          # (ceil: the decimated grid keeps row 64 and column 92)
    # boxes that force r = 0: smaller than twice the output, or magnified
    assert plan([(512, 768)], [(10, 20, 300, 300)], (224, 224)) == (0, [(10, 20, 300, 300)])
    assert plan([(512, 768)], [(3, 5, 100, 90)], (224, 224)) == (0, [(3, 5, 100, 90)])
    # the mapping keeps only grid pixels INSIDE the box: odd origin rounds up, the last pixel rounds down
    assert plan([(512, 768)], [(1, 3, 449, 450)], (224, 224)) == (1, [(1, 2, 224, 225)])
    assert plan([(512, 768)], [(1, 3, 447, 450)], (224, 224)) == (0, [(1, 3, 447, 450)])  # rows 2 .. 446: 223 < 224
    # a box whose mapped extent would be 0 at r >= 1 (one odd row, one odd column): r stays 0, for any output size
    assert plan([(64, 64)], [(5, 7, 1, 1)], (1, 1)) == (0, [(5, 7, 1, 1)])
    assert plan([(64, 64)], [(4, 8, 1, 1)], (1, 1)) == (2, [(1, 2, 1, 1)])                 # row 4 is on the grid up to r = 2
    # mixed sizes: one value for the call, set by the image that can afford least
    r, boxes = plan([(2160, 3840), (512, 768), (1080, 1920)], [(0, 0, 2160, 3840), (0, 0, 512, 768), (100, 200, 900, 900)], (224, 224))
    assert r == 1 and boxes == [(0, 0, 1080, 1920), (0, 0, 256, 384), (50, 100, 450, 450)]
    r, boxes = plan([(2160, 3840), (1080, 1920)], [(7, 9, 2001, 1999), (100, 200, 900, 900)], (224, 224))
    assert r == 2 and boxes == [(2, 3, 500, 499), (25, 50, 225, 225)]
    for (H, W), (y0, x0, h, w) in zip([(2160, 3840), (1080, 1920)], boxes):
        assert cd.resize_window_ok(H, W, r, y0, x0, h, w, 224, 224, True)                # what it returns is what the call takes
    with pytest.raises(ValueError):
        plan([(64, 64)], [(0, 0, 65, 64)], (8, 8))
    assert "decimation" in plan.__doc__.lower() and "aliases" in plan.__doc__.lower()


# ------------------------------------------------------------------------------------------------ the spec against torch
# (box h, w) -> (Ho, Wo), filter flag: down by exactly 4 (8 taps) and by 3.84 / 3.76 (9 taps), 2.3 x down with and without the filter, 1.7 x up,
# a tall box to a wide output, the identity, and a 1 x 1 box
SPEC_SHAPES = [((64, 96), (16, 24), 1), ((96, 64), (25, 17), 1), ((67, 93), (29, 40), 1), ((67, 93), (29, 40), 0), ((33, 32), (56, 54), 1),
               ((60, 20), (16, 48), 1), ((60, 20), (16, 48), 0), ((31, 33), (31, 33), 1), ((1, 1), (5, 7), 1), ((1, 1), (5, 7), 0)]
U = 2.0 ** -24


def spec_bound(hs, ws, Ho, Wo, antialias):
    """The largest difference, in 0 .. 255 pixel units, two fp32 evaluations of the filter may show: (rounded operations on a value's path,
    ours + torch's) x 2^-24 x 255.  Counting, per axis, with n the box extent, m the output extent, M = max(n, m) and T the tap count:
      - a tap's t_k goes through scale, center, k - center, + 0.5, * inv (inv itself is one more) and 1 - |.|: seven operations.  The first
        three carry an error relative to `center`, which is up to M tap spacings while t_k is at most 1: in units of 2^-24 of the weight they
        count as 3 M, the other four as 1 each.  torch evaluates the same expressions (its antialias kernel) or, without the filter, the shorter
        lerp form w1 = x - floor(x), w0 = 1 - w1 with the same source index path: 3 M + 4 bounds both.
      - w_k = t_k / total: T - 1 rounded additions and one division, and the error of t_k enters twice (numerator and total): 2 (3 M + 4) + T.
      - the pass itself: T products and T - 1 additions with |w| <= 1 and partial sums <= 255: 2 T - 1.
    A value passes the column axis, then the row axis.  torch is granted the same count as ours (it sums in another order and may contract
    a product into the sum, which removes roundings, never adds any)."""
    n_ops = 0
    for n, m in ((ws, Wo), (hs, Ho)):
        T = int(rr.axis_taps(n, m, antialias)[1].max())
        n_ops += 2 * (3 * max(n, m) + 4) + T + 2 * T - 1
    return 2 * n_ops * U * 255.0


def measure_against_torch():
    """-> [(shape, measured maximum, bound)] for SPEC_SHAPES: ref_resize.resample against F.interpolate in float32 on the CPU"""
    import torch.nn.functional as Fn
    out = []
    for k, ((hs, ws), (Ho, Wo), aa) in enumerate(SPEC_SHAPES):
        box = np.random.default_rng(100 + k).integers(0, 256, (3, hs, ws), dtype=np.uint8)
        mine = rr.resample(box, Ho, Wo, aa)
        ref = Fn.interpolate(torch.from_numpy(box.astype(np.float32))[None], size=(Ho, Wo), mode="bilinear", align_corners=False, antialias=bool(aa))[0].numpy()
        assert ref.dtype == np.float32 and ref.shape == mine.shape
        out.append((((hs, ws), (Ho, Wo), aa), float(np.abs(mine.astype(np.float64) - ref.astype(np.float64)).max()), spec_bound(hs, ws, Ho, Wo, aa)))
    return out


def test_spec_is_torch_interpolate_within_the_derived_bound():
    """ref_resize (the arithmetic the kernel is held to, bit for bit) against F.interpolate(mode="bilinear", align_corners=False, antialias=flag)
    in float32 on the CPU, on SPEC_SHAPES, within spec_bound (its docstring derives it: 0.003 .. 0.03 pixel units on these shapes; a wrong
    center, support or normalisation is off by a pixel unit or more).  Measured when written: at most 1.5e-4 (profiles/resized_decode/accuracy.json).
    At n == m the pixels come back exactly."""
    for shape, err, bound in measure_against_torch():
        print(shape, "max |ref_resize - torch| = %.3g, bound %.3g" % (err, bound))
        assert err <= bound, (shape, err, bound)
        assert bound < 0.05, shape
    box = np.random.default_rng(3).integers(0, 256, (3, 31, 33), dtype=np.uint8)
    for aa in (0, 1):
        assert np.array_equal(rr.resample(box, 31, 33, aa), box.astype(np.float32))
    rec = json.load(open(os.path.join(ROOT, "profiles", "resized_decode", "accuracy.json")))
    assert len(rec["shapes"]) == len(SPEC_SHAPES) and all(s["max_abs_diff_pixel_units"] <= s["bound_pixel_units"] for s in rec["shapes"])


def test_finish_is_torch_arithmetic():
    """ref_resize.finish -- / 255, normalise, dtype rounding -- against torch on the CPU, exactly (the steps unlift_tensor_kernel is held to)"""
    v = np.random.default_rng(9).uniform(0, 255, (3, 40, 50)).astype(np.float32)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    t = torch.from_numpy(v) / 255
    tn = (t - torch.tensor(mean)[:, None, None]) / torch.tensor(std)[:, None, None]
    for name, dt in (("float32", torch.float32), ("float16", torch.float16), ("bfloat16", torch.bfloat16)):
        assert np.array_equal(rr.finish(v, dtype=name), t.to(dt).float().numpy()), name
        assert np.array_equal(rr.finish(v, mean, std, dtype=name), tn.to(dt).float().numpy()), name


# ------------------------------------------------------------------------------------------------ host validation
def test_host_side_of_a_resized_call(tmp_path):
    """tests/sanitize_resize_host.cpp against llicti_amd/csrc/host_plan.hpp (g++, no HIP): box words, every NULL default, every refusal and its
    message.  Built plain here; the file's head says how to run it under AddressSanitizer + UBSan."""
    import subprocess
    exe = str(tmp_path / "sanitize_resize_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(HERE, "sanitize_resize_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert "resize boxes ok" in out.stdout


if __name__ == "__main__":
    # writes the record the spec test reads: PYTHONPATH=.:tests python tests/test_resize_cpu.py
    rows = measure_against_torch()
    rec = {"what": "tests/ref_resize.py (numpy float32) against torch.nn.functional.interpolate(bilinear, align_corners=False), float32, CPU",
           "torch": torch.__version__, "unit": "pixel units, 0 .. 255",
           "shapes": [{"box": list(s[0]), "out": list(s[1]), "antialias": s[2], "max_abs_diff_pixel_units": e, "bound_pixel_units": b} for s, e, b in rows],
           "max_abs_diff_pixel_units": max(e for _, e, _ in rows)}
    path = os.path.join(ROOT, "profiles", "resized_decode", "accuracy.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec, indent=1))
