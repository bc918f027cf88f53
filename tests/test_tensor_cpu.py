"""Float tensor surfaces, the parts that need no GPU: the new symbols are declared, exported and bound, and the two host helpers --
llicti_tensor_elem_bytes and llicti_tensor_window_ok, the latter over a grid of sizes, reduces, origins and window sizes against reduced_dims and
plain inequalities."""
import itertools
import os
import re

import pytest
import torch

from llicti_amd import _lib
from llicti_amd import codec as cd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ["llicti_tensor_elem_bytes", "llicti_tensor_window_ok", "llicti_decode_images_tensor", "llicti_encode_images_f32"]


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "llicti_hip.h")).read()
    L = _lib.lib()                       # (binds every name of _SIGS: a missing export raises here)
    for name in NEW:
        assert name in _lib.EXPORTS and re.search(r"\b%s\(" % name, header), name
        assert getattr(L, name).argtypes == _lib._SIGS[name][1]
        # the argument count the header declares
        decl = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(decl.split(",")) == len(_lib._SIGS[name][1]), name
    for k, (name, v) in enumerate((("LLICTI_T_F32", cd.T_F32), ("LLICTI_T_F16", cd.T_F16), ("LLICTI_T_BF16", cd.T_BF16))):
        assert v == k and re.search(r"#define %s %d\b" % (name, k), header), name
    assert cd.TENSOR_DTYPES == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def test_tensor_elem_bytes():
    L = _lib.lib()
    assert [L.llicti_tensor_elem_bytes(d) for d in range(3)] == [4, 2, 2]
    for dt in cd.TENSOR_DTYPES:
        assert cd.tensor_elem_bytes(dt) == torch.empty((), dtype=dt).element_size()
    for bad in (-1, 3, 7, 100):
        assert L.llicti_tensor_elem_bytes(bad) == 0
        with pytest.raises(ValueError):
            cd.tensor_elem_bytes(bad)


def test_tensor_window_ok_against_plain_inequalities():
    L = _lib.lib()
    n = 0
    for (H, W), r in itertools.product(((32, 32), (33, 35), (67, 93), (64, 96), (512, 768), (8160, 8160)), range(6)):
        Hr, Wr = cd.reduced_dims(H, W, r)
        sizes = {(1, 1), (Hr, Wr), (Hr, 1), (1, Wr), (max(1, Hr // 2), max(1, Wr // 3)), (Hr + 1, Wr), (Hr, Wr + 1)}
        for Ho, Wo in sizes:
            # origins: the corner, the last legal one (the window touches the bottom / right edge), one past it, and a negative one
            ys = {0, 1, Hr - Ho, Hr - Ho + 1, (Hr - Ho) // 2, -1}
            xs = {0, 1, Wr - Wo, Wr - Wo + 1, (Wr - Wo) // 2, -1}
            for y0, x0 in itertools.product(ys, xs):
                want = 0 <= y0 and y0 + Ho <= Hr and 0 <= x0 and x0 + Wo <= Wr
                assert L.llicti_tensor_window_ok(H, W, r, y0, x0, Ho, Wo) == int(want), (H, W, r, y0, x0, Ho, Wo)
                assert cd.tensor_window_ok(H, W, r, y0, x0, Ho, Wo) is want
                n += 1
    assert n > 3000                      # (the grid did not collapse)
    # the edges by name, on 67 x 93 at reduce 1 (34 x 47)
    assert L.llicti_tensor_window_ok(67, 93, 1, 2, 15, 32, 32) == 1          # touches bottom and right
    assert L.llicti_tensor_window_ok(67, 93, 1, 3, 15, 32, 32) == 0          # one row too far
    assert L.llicti_tensor_window_ok(67, 93, 1, 2, 16, 32, 32) == 0          # one column too far
    assert L.llicti_tensor_window_ok(33, 35, 1, 0, 0, 32, 32) == 0           # 17 x 18 holds no 32 x 32 window
    # arguments outside the domain
    for bad in ((0, 32, 0, 0, 0, 1, 1), (32, 0, 0, 0, 0, 1, 1), (32, 32, -1, 0, 0, 1, 1), (32, 32, 6, 0, 0, 1, 1), (32, 32, 0, 0, 0, 0, 1),
                (32, 32, 0, 0, 0, 1, 0), (32, 32, 0, 0, 0, -4, 4), (32, 32, 0, 2 ** 31 - 1, 0, 2, 2)):
        assert L.llicti_tensor_window_ok(*bad) == 0, bad


def test_host_side_of_a_tensor_call(tmp_path):
    """tests/sanitize_tensor_host.cpp against llicti_amd/csrc/host_plan.hpp (g++, no HIP): window words, refusals and their messages.  Built plain
    here; the file's head says how to run it under AddressSanitizer + UBSan."""
    import subprocess
    exe = str(tmp_path / "sanitize_tensor_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(HERE, "sanitize_tensor_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert "tensor windows ok" in out.stdout
