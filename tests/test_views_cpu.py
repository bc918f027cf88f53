"""Views, the parts that need no GPU: codec.multi_crop_plan against a brute-force restatement, the ctypes structure of a group against the C
compiler's layout of llicti_view_group, the header as C99, and the host validation (resolve_views) compiled by g++ into a stand-alone driver."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from llicti_amd import _lib
from llicti_amd import codec as cd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER_DIR = os.path.join(ROOT, "include")
FIELDS = ["d_out", "dtype", "Ho", "Wo", "antialias", "n", "image", "y0", "x0", "hs", "ws", "flip"]


def test_new_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(HEADER_DIR, "llicti_hip.h")).read()
    name = "llicti_decode_images_tensor_views"
    assert name in _lib.EXPORTS and re.search(r"\b%s\(" % name, header)
    decl = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1)
    assert len(decl.split(",")) == len(_lib._SIGS[name][1]) == len(getattr(_lib.lib(), name).argtypes)
    assert _lib._SIGS[name][1][12] is C.POINTER(_lib.ViewGroup)
    assert int(re.search(r"#define LLICTI_VIEW_GROUPS_MAX (\d+)", header).group(1)) == _lib.VIEW_GROUPS_MAX == 16
    assert cd.VIEW_SLICE == 128


# ------------------------------------------------------------------------------------------------ the structure
def test_ctypes_group_has_the_c_compilers_layout(tmp_path):
    """sizeof and every offsetof of llicti_view_group, printed by a C99 program compiled against the header, equal the ctypes.Structure's"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "llicti_hip.h"\nint main(void)\n{\n'
                   '    printf("%zu", sizeof(llicti_view_group));\n'
                   + "".join('    printf(" %%zu", offsetof(llicti_view_group, %s));\n' % f for f in FIELDS)
                   + '    printf("\\n");\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", HEADER_DIR, "-o", exe, str(src)])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert [f for f, _ in _lib.ViewGroup._fields_] == FIELDS
    assert got == [C.sizeof(_lib.ViewGroup)] + [getattr(_lib.ViewGroup, f).offset for f in FIELDS], got


# ------------------------------------------------------------------------------------------------ multi_crop_plan
def brute_plan(sizes, groups_full, nlevels=5):
    """multi_crop_plan restated pixel by pixel: at reduce r the decoded grid holds the pixels whose row and column are multiples of 2^r; a view keeps
    those INSIDE its full-resolution box; r is the largest at which every view keeps at least Ho rows and Wo columns"""
    def kept(lo, n, s):
        idx = [k // s for k in range(lo, lo + n) if k % s == 0]
        return (idx[0], len(idx)) if idx else (-(-lo // s), 0)

    def at(r):
        res = []
        for (Ho, Wo), image, boxes in groups_full:
            rows = []
            for y0, x0, h, w in boxes:
                (yr, hr), (xr, wr) = kept(y0, h, 1 << r), kept(x0, w, 1 << r)
                rows.append((yr, xr, hr, wr))
            res.append(rows)
        return res

    for (Ho, Wo), image, boxes in groups_full:
        image = range(len(sizes)) if image is None else image
        for b, (y0, x0, h, w) in zip(image, boxes):
            if not (0 <= b < len(sizes) and y0 >= 0 and x0 >= 0 and h >= 1 and w >= 1 and y0 + h <= sizes[b][0] and x0 + w <= sizes[b][1]):
                raise ValueError
    best = 0
    for r in range(1, nlevels + 1):
        if all(hr >= Ho and wr >= Wo for ((Ho, Wo), _, _), rows in zip(groups_full, at(r)) for _, _, hr, wr in rows):
            best = r
    return best, at(best)


def test_multi_crop_plan_against_brute_force():
    rng = np.random.default_rng(2026)
    seen = set()
    for _ in range(300):
        B = int(rng.integers(1, 5))
        sizes = [(int(rng.integers(32, 700)), int(rng.integers(32, 700))) for _ in range(B)]
        nlev = int(rng.choice([2, 5]))
        groups = []
        for _g in range(int(rng.integers(1, 4))):
            size = (int(rng.integers(1, 120)), int(rng.integers(1, 120)))
            ident = bool(rng.integers(0, 4) == 0)
            image = None if ident else [int(v) for v in rng.integers(0, B, int(rng.integers(1, 7)))]
            boxes = []
            for b in (range(B) if ident else image):
                H, W = sizes[b]
                h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
                boxes.append((int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w))
            groups.append((size, image, boxes))
        got = cd.multi_crop_plan(sizes, groups, nlevels=nlev)
        assert got == brute_plan(sizes, groups, nlev), (sizes, groups, nlev)
        seen.add(got[0])
        r, mapped = got
        for (size, image, _), boxes in zip(groups, mapped):       # what it returns is what the call takes (no filter: the scale may exceed 4)
            for b, (y0, x0, h, w) in zip(range(B) if image is None else image, boxes):
                assert cd.resize_window_ok(sizes[b][0], sizes[b][1], r, y0, x0, h, w, size[0], size[1], False), (sizes[b], r, (y0, x0, h, w))
    assert len(seen) >= 4                                         # (the draw reached several values of reduce)


def test_multi_crop_plan_by_hand():
    plan = cd.multi_crop_plan
    sizes = [(768, 512), (2160, 3840)]
    # the small crops decide: a 224 output of a 700 x 500 box could run at r = 1, a 96 output of a 150 x 150 box cannot (75 < 96)
    big = ((224, 224), [0, 1], [(10, 6, 700, 500), (0, 0, 2160, 3840)])
    assert plan(sizes, [big]) == (1, [[(5, 3, 350, 250), (0, 0, 1080, 1920)]])
    small = ((96, 96), [0, 0, 1], [(100, 100, 150, 150), (1, 3, 449, 450), (7, 9, 2001, 1999)])
    assert plan(sizes, [big, small]) == (0, [list(big[2]), list(small[2])])
    small2 = ((64, 64), [0, 0, 1], small[2])
    assert plan(sizes, [big, small2]) == (1, [[(5, 3, 350, 250), (0, 0, 1080, 1920)], [(50, 50, 75, 75), (1, 2, 224, 225), (4, 5, 1000, 999)]])
    assert plan(sizes, [big, small2], nlevels=0)[0] == 0
    # images no view names, repeats, any order
    assert plan(sizes, [((8, 8), [1, 1, 1], [(0, 0, 64, 64), (64, 64, 64, 64), (1, 1, 64, 64)])]) == (3, [[(0, 0, 8, 8), (8, 8, 8, 8), (1, 1, 8, 8)]])
    for bad in ([((8, 8), [0], [(0, 0, 769, 8)])], [((8, 8), [1, 0], [(0, 0, 8, 8), (0, 0, 8, 513)])], [((8, 8), [0], [(-1, 0, 8, 8)])],
                [((8, 8), [0], [(0, 0, 0, 8)])], [((8, 8), [2], [(0, 0, 8, 8)])], [((8, 8), [-1], [(0, 0, 8, 8)])],
                [((8, 8), None, [(0, 0, 8, 8), (0, 0, 2161, 8)])]):
        with pytest.raises(ValueError):
            plan(sizes, bad)
    assert "decimation" in plan.__doc__.lower() and "aliases" in plan.__doc__.lower()


def test_one_identity_group_is_resized_crop_plan():
    rng = np.random.default_rng(7)
    for _ in range(200):
        B = int(rng.integers(1, 6))
        sizes = [(int(rng.integers(32, 3000)), int(rng.integers(32, 3000))) for _ in range(B)]
        boxes = []
        for H, W in sizes:
            h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
            boxes.append((int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w))
        size = (int(rng.integers(1, 300)), int(rng.integers(1, 300)))
        nlev = int(rng.choice([2, 5]))
        r, mapped = cd.resized_crop_plan(sizes, boxes, size, nlevels=nlev)
        assert cd.multi_crop_plan(sizes, [(size, None, boxes)], nlevels=nlev) == (r, [mapped])
        assert cd.multi_crop_plan(sizes, [(size, list(range(B)), boxes)], nlevels=nlev) == (r, [mapped])
    with pytest.raises(ValueError):
        cd.multi_crop_plan([(64, 64)], [((8, 8), None, [(0, 0, 65, 64)])])


# ------------------------------------------------------------------------------------------------ host validation
def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "llicti_hip.h"\nint main(void) { llicti_view_group g; (void)g; return LLICTI_VIEW_GROUPS_MAX == 16 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", HEADER_DIR, "-o", str(tmp_path / "h"), str(src)])
    assert subprocess.run([str(tmp_path / "h")]).returncode == 0


def test_host_side_of_a_views_call(tmp_path):
    """tests/sanitize_views_host.cpp against llicti_amd/csrc/host_plan.hpp (g++, no HIP): view words, every NULL default, every refusal and its
    message, image index 65,535 and 1,048,576 views.  Built plain here; the file's head says how to run it under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "sanitize_views_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(HERE, "sanitize_views_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert "view tables ok" in out.stdout
