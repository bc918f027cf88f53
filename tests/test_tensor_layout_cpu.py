"""Tensor options, the parts that need no GPU: the five new symbols are declared, exported and bound; llicti_pad_index -- compiled from the function
the kernel calls -- against tests/ref_pad.py, np.pad and torch's F.pad; llicti_tensor_window_pad_ok against brute force; center_crop_origins
against explicit pad-then-crop; the host side of the calls under AddressSanitizer + UBSan (tests/sanitize_tensor_opts_host.cpp, a program of its
own); and the new kernels' resources from hipcc's metadata."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ref_pad
from llicti_amd import _lib
from llicti_amd import codec as cd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ["llicti_pad_index", "llicti_tensor_window_pad_ok", "llicti_decode_images_tensor_o", "llicti_decode_images_tensor_resized_o",
       "llicti_decode_images_tensor_views_o"]
MODES = {"constant": 1, "edge": 2, "reflect": 3, "symmetric": 4}


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "llicti_hip.h")).read()
    L = _lib.lib()                       # (binds every name of _SIGS: a missing export raises here)
    for name in NEW:
        assert name in _lib.EXPORTS and re.search(r"\b%s\(" % name, header), name
        assert getattr(L, name).argtypes == _lib._SIGS[name][1]
        decl = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(decl.split(",")) == len(_lib._SIGS[name][1]), name
    # the _o calls are their _rv siblings with one more argument: the options, last
    for stem in ("llicti_decode_images_tensor", "llicti_decode_images_tensor_resized", "llicti_decode_images_tensor_views"):
        assert _lib._SIGS[stem + "_o"][1][:-1] == _lib._SIGS[stem + "_rv"][1] and _lib._SIGS[stem + "_o"][1][-1] == C.POINTER(_lib.TensorOpts)
    for name, v in (("LLICTI_LAYOUT_NCHW", cd.LAYOUT_NCHW), ("LLICTI_LAYOUT_NHWC", cd.LAYOUT_NHWC), ("LLICTI_PAD_NONE", cd.PAD_NONE),
                    ("LLICTI_PAD_CONSTANT", cd.PAD_CONSTANT), ("LLICTI_PAD_EDGE", cd.PAD_EDGE), ("LLICTI_PAD_REFLECT", cd.PAD_REFLECT),
                    ("LLICTI_PAD_SYMMETRIC", cd.PAD_SYMMETRIC), ("LLICTI_FILL_PIXEL", cd.FILL_PIXEL), ("LLICTI_FILL_OUTPUT", cd.FILL_OUTPUT)):
        assert re.search(r"#define %s %d\b" % (name, v), header), name
    assert cd.PAD_MODES == MODES and (cd.PAD_NONE, cd.LAYOUT_NHWC, cd.FILL_OUTPUT) == (0, 1, 1)
    assert (ref_pad.NONE, ref_pad.CONSTANT, ref_pad.EDGE, ref_pad.REFLECT, ref_pad.SYMMETRIC) == (0, 1, 2, 3, 4)
    # the struct as the header lays it out: three ints and three floats
    assert re.search(r"typedef struct llicti_tensor_opts \{ int layout, pad_mode, fill_space; float fill\[3\]; \} llicti_tensor_opts;", header)
    assert [f[0] for f in _lib.TensorOpts._fields_] == ["layout", "pad_mode", "fill_space", "fill"] and C.sizeof(_lib.TensorOpts) == 24


def _limit(mode, n):
    """the largest overhang a mode mirrors on an axis of n (None: no limit)"""
    return {"reflect": n - 1, "symmetric": n}.get(mode)


def test_pad_index_is_the_reference_and_numpy():
    """Every mode, n in 1 .. 9, every overhang up to the mode's limit and one beyond (constant / edge: up to n + 2): the library's index equals
    ref_pad's, and equals the index pattern np.pad leaves when it pads np.arange(n); one beyond the limit is refused."""
    L = _lib.lib()
    checked = 0
    for mode, code in MODES.items():
        for n in range(1, 10):
            lim = _limit(mode, n)
            top = n + 2 if lim is None else lim
            for over in range(0, top + 1):
                if over == 0:
                    want = np.arange(n)
                elif mode == "constant":
                    want = np.pad(np.arange(n), over, mode="constant", constant_values=-1)
                else:
                    want = np.pad(np.arange(n), over, mode=mode)
                got = [L.llicti_pad_index(n, t, code) for t in range(-over, n + over)]
                assert got == list(want), (mode, n, over)
                assert got == [ref_pad.pad_index(n, t, mode) for t in range(-over, n + over)] == [cd.pad_index(n, t, mode) for t in range(-over, n + over)]
                checked += len(got)
            if lim is not None:              # one beyond: refused, on either side, by both readings
                for t in (-(lim + 1), n - 1 + lim + 1):
                    assert L.llicti_pad_index(n, t, code) == -2 == ref_pad.pad_index(n, t, mode), (mode, n, t)
                    assert L.llicti_pad_index(n, t + (1 if t < 0 else -1), code) >= 0 or lim == 0, (mode, n, t)
    assert checked > 1500
    # no pad mode: inside or refused; outside the domain
    for n, t in itertools.product(range(1, 6), range(-3, 9)):
        assert L.llicti_pad_index(n, t, 0) == (t if 0 <= t < n else -2) == ref_pad.pad_index(n, t, 0)
    for bad in ((0, 0, 2), (-4, 0, 1), (8161, 0, 2), (4, 0, 5), (4, 0, -1), (4, 2 ** 21, 2), (4, -2 ** 21, 1)):
        assert L.llicti_pad_index(*bad) == -2, bad
    assert L.llicti_pad_index(8160, -8160, 4) == 8159 and L.llicti_pad_index(8160, 8160 + 8159, 4) == 0 and L.llicti_pad_index(8160, -8159, 3) == 8159


def test_pad_index_is_torch_pad_for_reflect_and_replicate():
    L = _lib.lib()
    for n in range(2, 10):
        x = torch.arange(n, dtype=torch.float32)[None, None, :]
        for mode, tmode in (("reflect", "reflect"), ("edge", "replicate")):
            for lo, hi in itertools.product(range(0, n), repeat=2):
                want = torch.nn.functional.pad(x, (lo, hi), mode=tmode)[0, 0].to(torch.int64).tolist()
                assert [L.llicti_pad_index(n, t, MODES[mode]) for t in range(-lo, n + hi)] == want, (mode, n, lo, hi)
        with pytest.raises(RuntimeError):        # torch refuses what the library refuses: a reflection of n pixels past a side of n
            torch.nn.functional.pad(x, (n, 0), mode="reflect")
        assert L.llicti_pad_index(n, -n, MODES["reflect"]) == -2


def test_tensor_window_pad_ok_against_brute_force():
    L = _lib.lib()
    n = 0
    for (H, W), r, mode in itertools.product(((3, 5), (4, 4), (1, 7), (9, 2)), (0, 1, 2), (0, 1, 2, 3, 4)):
        Hr, Wr = (H + (1 << r) - 1) >> r, (W + (1 << r) - 1) >> r
        assert (Hr, Wr) == cd.reduced_dims(H, W, r)
        for Ho, Wo in ((1, 1), (2, 3), (Hr, Wr), (Hr + 1, Wr + 2), (2 * Hr, 2 * Wr + 1), (3 * Hr + 1, 1)):
            for y0, x0 in itertools.product(range(-2 * Hr - 1, 2 * Hr + 2, max(1, Hr // 2)), range(-2 * Wr - 1, 2 * Wr + 2, max(1, Wr // 2))):
                want = ref_pad.window_ok(Hr, Wr, y0, x0, Ho, Wo, mode)
                assert L.llicti_tensor_window_pad_ok(H, W, r, y0, x0, Ho, Wo, mode) == int(want), (H, W, r, y0, x0, Ho, Wo, mode)
                if mode == 0:
                    assert want == bool(L.llicti_tensor_window_ok(H, W, r, y0, x0, Ho, Wo))
                n += 1
    assert n > 5000
    assert cd.tensor_window_pad_ok(67, 93, 0, -6, -9, 80, 112, "reflect") and not cd.tensor_window_pad_ok(67, 93, 0, -67, 0, 80, 112, "reflect")
    assert cd.tensor_window_pad_ok(67, 93, 0, -67, -93, 80, 112, "symmetric") and not cd.tensor_window_pad_ok(67, 93, 0, -68, 0, 80, 112, "symmetric")
    assert cd.tensor_window_pad_ok(67, 93, 0, 500, -500, 80, 112, "constant") and cd.tensor_window_pad_ok(67, 93, 2, -8160, 8160, 8160, 8160, "edge")
    for bad in ((67, 93, 0, -8161, 0, 4, 4, 1), (67, 93, 0, 0, 8161, 4, 4, 2), (67, 93, 0, 0, 0, 8161, 4, 1), (67, 93, 0, 0, 0, 4, 0, 2),
                (67, 93, 6, 0, 0, 4, 4, 1), (67, 93, -1, 0, 0, 4, 4, 1), (0, 93, 0, 0, 0, 4, 4, 1), (67, 93, 0, 0, 0, 4, 4, 5), (67, 93, 0, 0, 0, 4, 4, -1)):
        assert L.llicti_tensor_window_pad_ok(*bad) == 0, bad


def test_center_crop_origins_are_pad_then_crop():
    """torchvision's CenterCrop, image by image, on np.arange grids: pad (c - n) // 2 in front and (c - n + 1) // 2 behind where n < c, then cut c
    from int(round((n' - c) / 2.0)) -- the window center_crop_origins names, read through the constant pad's index map, shows the same
    coordinates.  Sizes smaller than the crop, equal to it and larger, odd and even differences."""
    crop = (48, 37)
    sizes = [(h, w) for h in (40, 41, 47, 48, 49, 50, 96, 131) for w in (33, 36, 37, 38, 60, 61)]
    for reduce in (0, 1, [k % 3 for k in range(len(sizes))]):
        y0s, x0s = cd.center_crop_origins(sizes, crop, reduce)
        rs = [reduce] * len(sizes) if isinstance(reduce, int) else reduce
        for (H, W), r, y0, x0 in zip(sizes, rs, y0s, x0s):
            for n, c, o in ((cd.reduced_dims(H, W, r)[0], crop[0], y0), (cd.reduced_dims(H, W, r)[1], crop[1], x0)):
                grid = np.arange(n)
                if n < c:
                    grid = np.pad(grid, ((c - n) // 2, (c - n + 1) // 2), mode="constant", constant_values=-1)
                start = int(round((len(grid) - c) / 2.0))
                want = grid[start:start + c]
                assert len(want) == c
                assert [ref_pad.pad_index(n, o + k, "constant") for k in range(c)] == list(want), (H, W, r, n, c, o)
    assert cd.center_crop_origins([(40, 60), (150, 131)], (48, 48)) == ([-4, 51], [6, 42])
    assert cd.center_crop_origins([(40, 60)], (48, 48), reduce=[1]) == ([-14], [-9])


def test_host_side_of_the_option_calls_under_sanitizers(tmp_path):
    """tests/sanitize_tensor_opts_host.cpp against llicti_amd/csrc/host_plan.hpp (g++, no HIP), with AddressSanitizer and UBSan: validation and
    packing over a few thousand option / window combinations, the limits among them."""
    exe = str(tmp_path / "sanitize_tensor_opts_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HERE, "sanitize_tensor_opts_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    m = re.search(r"tensor options ok: (\d+) checks", out.stdout)
    assert m and int(m.group(1)) > 3000, out.stdout


def test_new_kernels_have_no_scratch_and_the_old_ones_are_all_there():
    """hipcc's metadata of the device code (tools/kernel_resources.py; no GPU needed): three element types of each of the three new sinks, none
    with a private segment, a spilled vector register or a dynamic stack; and the five older sinks are the instantiations they were."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources()
    new = [r for r in rows if re.match(r"_Z\d+sink_(window|resize_nhwc|views_nhwc)_kernel", r["name"])]
    assert len(new) == 3 * 3, [r["name"] for r in new]
    for r in new:
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and not r["uses_dynamic_stack"], r
    old = [r for r in rows if re.match(r"_Z\d+unlift_(reduced|px|tensor|resize_tensor|views_tensor)_kernel", r["name"])]
    assert len(old) == 2 + 3 * 3, [r["name"] for r in old]
