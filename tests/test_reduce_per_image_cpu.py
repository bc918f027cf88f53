"""Per-image reduce, the parts that need no GPU: the planners' per_image=True against a brute-force count of np.arange(n)[::2^r] inside the box,
the five new symbols (header, library, bindings), the per-call schedule of host_plan.hpp driven by a stand-alone program under AddressSanitizer
and UBSan, and the resources of the kernels the feature touched against the parent's (profiles/per_image_reduce/kernel_resources_parent.json,
tools/kernel_resources.py's output on the commit before this feature)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from llicti_amd import _lib
from llicti_amd import codec as cd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RV = ["llicti_decode_images_reduced_rv", "llicti_decode_images_px_rv", "llicti_decode_images_tensor_rv", "llicti_decode_images_tensor_resized_rv",
      "llicti_decode_images_tensor_views_rv"]


# ------------------------------------------------------------------------------------------------ symbols
def test_new_symbols_are_declared_exported_and_bound():
    """Each _rv call is its scalar sibling with `int reduce` (argument 9) replaced by a pointer: in the header, in the built library, in _lib.py."""
    header = open(os.path.join(ROOT, "include", "llicti_hip.h")).read()
    L = _lib.lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    for name in RV:
        sib = name[:-3]
        assert name in _lib.EXPORTS and re.search(r"\b%s\(" % name, header), name
        assert re.search(r" T %s$" % name, syms, re.M), (name, "not exported by the built library")
        decl = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1).split(",")
        sdecl = re.search(r"int %s\((.*?)\);" % sib, header, re.S).group(1).split(",")
        assert len(decl) == len(sdecl) == len(_lib._SIGS[name][1]) == len(getattr(L, name).argtypes), name
        assert decl[9].strip() == "const int *reduces" and sdecl[9].strip() == "int reduce", (decl[9], sdecl[9])
        assert [a.strip() for k, a in enumerate(decl) if k != 9] == [a.strip() for k, a in enumerate(sdecl) if k != 9], name
        a, b = _lib._SIGS[name][1], _lib._SIGS[sib][1]
        assert a[9] is _lib._vp and b[9] is _lib._i and a[:9] + a[10:] == b[:9] + b[10:], name


# ------------------------------------------------------------------------------------------------ planners
def kept(lo, n, r):
    """the pixels of the grid decimated by 2^r that lie inside [lo, lo + n): (index of the first on that grid, how many) -- counted, not computed"""
    grid = np.arange(8192)[::1 << r]
    inside = np.nonzero((grid >= lo) & (grid < lo + n))[0]
    return (int(inside[0]), len(inside)) if len(inside) else (None, 0)


def brute_r(box, size, nlevels):
    y0, x0, h, w = box
    best = 0
    for r in range(1, nlevels + 1):
        if kept(y0, h, r)[1] >= size[0] and kept(x0, w, r)[1] >= size[1]:
            best = r
    return best


def brute_box(box, r):
    y0, x0, h, w = box
    (yr, hr), (xr, wr) = kept(y0, h, r), kept(x0, w, r)
    return (yr, xr, hr, wr)


def _draw(rng, n):
    sizes = [(int(rng.integers(32, 900)), int(rng.integers(32, 900))) for _ in range(n)]
    boxes = []
    for H, W in sizes:
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        boxes.append((int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w))
    return sizes, boxes


@pytest.mark.parametrize("nlevels", [5, 2])
def test_resized_crop_plan_per_image_against_brute_force(nlevels):
    rng = np.random.default_rng(2026 + nlevels)
    seen = set()
    for _ in range(150):
        n = int(rng.integers(1, 9))
        sizes, boxes = _draw(rng, n)
        size = (int(rng.integers(1, 64)), int(rng.integers(1, 64)))
        rs, out = cd.resized_crop_plan(sizes, boxes, size, nlevels, per_image=True)
        want = [brute_r(b, size, nlevels) for b in boxes]
        assert rs == want, (sizes, boxes, size)
        for b, r, o in zip(boxes, rs, out):
            assert o == brute_box(b, r) and (o[2] >= size[0] and o[3] >= size[1] or r == 0), (b, r, o)
        seen.update(rs)
        # the default is what it was: ONE value, the smallest of the images', every box on that grid
        r1, out1 = cd.resized_crop_plan(sizes, boxes, size, nlevels)
        assert isinstance(r1, int) and r1 == min(want) and out1 == [brute_box(b, r1) for b in boxes]
        assert (r1, out1) == cd.resized_crop_plan(sizes, boxes, size, nlevels, per_image=False)
    assert seen == set(range(nlevels + 1))
    with pytest.raises(ValueError):
        cd.resized_crop_plan([(64, 64)], [(0, 0, 65, 64)], (8, 8), per_image=True)


@pytest.mark.parametrize("nlevels", [5, 2])
def test_multi_crop_plan_per_image_against_brute_force(nlevels):
    rng = np.random.default_rng(4052 + nlevels)
    unnamed = 0
    for _ in range(120):
        B = int(rng.integers(1, 7))
        sizes = [(int(rng.integers(32, 900)), int(rng.integers(32, 900))) for _ in range(B)]
        groups = []
        for g in range(int(rng.integers(1, 4))):
            size = (int(rng.integers(1, 48)), int(rng.integers(1, 48)))
            image = None if (g == 0 and rng.integers(0, 3) == 0) else [int(v) for v in rng.integers(0, B, int(rng.integers(1, 9)))]
            boxes = []
            for b in (range(B) if image is None else image):
                H, W = sizes[b]
                h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
                boxes.append((int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w))
            groups.append((size, image, boxes))
        rs, out = cd.multi_crop_plan(sizes, groups, nlevels, per_image=True)
        want = [nlevels] * B
        for size, image, boxes in groups:
            for b, box in zip(range(B) if image is None else image, boxes):
                want[b] = min(want[b], brute_r(box, size, nlevels))
        named = {b for _, image, _ in groups for b in (range(B) if image is None else image)}
        unnamed += B - len(named)
        assert rs == want and all(rs[b] == nlevels for b in range(B) if b not in named), (sizes, groups)
        for (size, image, boxes), got in zip(groups, out):
            assert got == [brute_box(box, rs[b]) for b, box in zip(range(B) if image is None else image, boxes)]
        r1, out1 = cd.multi_crop_plan(sizes, groups, nlevels)
        assert isinstance(r1, int) and r1 == min(want[b] for b in named)
        assert out1 == [[brute_box(box, r1) for box in boxes] for _, _, boxes in groups]
        assert (r1, out1) == cd.multi_crop_plan(sizes, groups, nlevels, per_image=False)
    assert unnamed > 0
    # one group over every image in order: resized_crop_plan's answer
    sizes, boxes = _draw(np.random.default_rng(9), 5)
    assert cd.multi_crop_plan(sizes, [((9, 11), None, boxes)], per_image=True) == (lambda r, b: (r, [b]))(*cd.resized_crop_plan(sizes, boxes, (9, 11), per_image=True))


def test_reduce_argument_of_the_wrappers():
    assert cd._reduce_arg(3, 4) == (3, None) and cd._reduce_arg(np.int64(0), 1) == (0, None)
    r, rv = cd._reduce_arg([0, 5, 2], 3)
    assert r is None and rv.dtype == np.int32 and rv.tolist() == [0, 5, 2] and rv.flags["C_CONTIGUOUS"]
    assert cd._reduce_arg(np.array([1, 1]), 2)[1].tolist() == [1, 1]
    with pytest.raises(ValueError):
        cd._reduce_arg([0, 1], 3)
    assert cd._reduced_sizes([67, 64], [93, 48], None, [5, 0]) == [(3, 3), (64, 48)]
    assert cd._reduced_sizes([67, 64], [93, 48], 1, None) == [(34, 47), (32, 24)]
    assert cd._reduced_sizes([67], [93], None, [9]) == [(67, 93)]          # (a value the library refuses: no exception here, the call says so)


# ------------------------------------------------------------------------------------------------ the schedule, under sanitizers
def test_schedule_driver_under_asan_and_ubsan(tmp_path):
    """tests/sanitize_reduce_rv_host.cpp over host_plan.hpp: g++ with AddressSanitizer + UBSan, run directly (its head lists what it holds)."""
    exe = str(tmp_path / "sanitize_reduce_rv_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HERE, "sanitize_reduce_rv_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    m = re.search(r"per-image reduce schedules ok: (\d+) batches \((\d+) all equal, (\d+) without a level-0 image\)", out.stdout)
    assert m and int(m.group(1)) >= 2000 and int(m.group(2)) > 100 and int(m.group(3)) > 100, out.stdout


# ------------------------------------------------------------------------------------------------ kernel resources
def _key(name):
    """a stage / tail kernel's identity without its parameter list (which grew by the level's stream list): base name and the lane-kind argument"""
    m = re.match(r"_Z\d+(rans_decode_stage_kernel|rans_decode_stage_pair_kernel|rans_decode_stage_lane_kernel|rans_tail_kernel)(?:ILi(\d+)EEv|P)", name)      # (a template's name carries its return type)
    return m and (m.group(1), m.group(2))


def test_kernels_keep_their_registers_and_have_no_scratch():
    """hipcc's metadata of the device code (tools/kernel_resources.py; no GPU needed): the five sinks, the three stage decoders and the tail
    kernel have no private segment and spill no vector register; the stage and tail kernels -- the SAME instantiations run the scalar calls,
    with a null list -- have no more VGPRs, no more spilled SGPRs and no more LDS than the parent's."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources()
    parent = json.load(open(os.path.join(ROOT, "profiles", "per_image_reduce", "kernel_resources_parent.json")))
    sinks = [r for r in rows if re.match(r"_Z\d+unlift_(reduced|px|tensor|resize_tensor|views_tensor)_kernel", r["name"])]
    assert len(sinks) == 2 + 3 * 3, [r["name"] for r in sinks]                 # planar, pixels, three tensor kernels x three element types
    stage = {_key(r["name"]): r for r in rows if _key(r["name"])}
    was = {_key(r["name"]): r for r in parent if _key(r["name"])}
    assert set(stage) == set(was) and len(stage) == 6, (sorted(stage), sorted(was))      # stage, pair, lane<4>, tail<1, 2, 4>
    for r in sinks + list(stage.values()):
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and not r["uses_dynamic_stack"], r
    for k, r in stage.items():
        p = was[k]
        assert r["vgpr_count"] <= p["vgpr_count"] and r["agpr_count"] <= p["agpr_count"], (k, r, p)
        assert r["sgpr_spill_count"] <= p["sgpr_spill_count"] and r["group_segment_fixed_size"] <= p["group_segment_fixed_size"], (k, r, p)
    one = [r for r in sinks if "unlift_reduced_kernel" in r["name"]]
    assert len(one) == 1 and one[0]["vgpr_count"] <= 32 and one[0]["group_segment_fixed_size"] == 0
