"""Transcode, the parts that need no GPU: llicti_transcode_workspace_bytes (it takes a NULL context: config A) against the sizes of the source-only
and target-only calls and over every combination the call refuses, the CLI's `transcode`, and the host layout of the two plans of a call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from llicti_amd import _lib
from llicti_amd.codec import MODE_AC, MODE_RANS, MODE_RANS_AUTO, auto_modes

HERE = os.path.dirname(os.path.abspath(__file__))


def _arr(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def _p(a):
    return C.c_void_p(a.ctypes.data)


def need(sizes, src, dst, ctx=None):
    """llicti_transcode_workspace_bytes; src / dst: one mode or a list with one per image"""
    Hs, Ws = _arr([h for h, _ in sizes]), _arr([w for _, w in sizes])
    s, d = _arr([src] if isinstance(src, (int, np.integer)) else src), _arr([dst] if isinstance(dst, (int, np.integer)) else dst)
    return int(_lib.lib().llicti_transcode_workspace_bytes(ctx, len(sizes), _p(Hs), _p(Ws), _p(s), len(s), _p(d), len(d)))


def alone(sizes, mode):
    Hs, Ws = _arr([h for h, _ in sizes]), _arr([w for _, w in sizes])
    if isinstance(mode, (int, np.integer)):
        return int(_lib.lib().llicti_workspace_bytes_v(len(sizes), _p(Hs), _p(Ws), int(mode)))
    return int(_lib.lib().llicti_workspace_bytes_vm(len(sizes), _p(Hs), _p(Ws), _p(_arr(mode))))


X = lambda m: MODE_RANS(m, wide=2)      # noqa: E731
KINDS = [MODE_AC, MODE_RANS(8), MODE_RANS(4, wide=1), X(2), X(10)]
MIXED = [(192, 256), (128, 192), (321, 481)]


@pytest.mark.parametrize("sizes", [[(67, 93)] * 2, [(96, 128)] * 2, [(32, 32)], [(768, 512)] * 24])
def test_workspace_covers_both_sides(sizes):
    for src in KINDS:
        for dst in KINDS + [MODE_RANS_AUTO(3)]:
            n = need(sizes, src, dst)
            a, b = alone(sizes, src), alone(sizes, dst)
            assert a > 0 and b > 0
            assert n >= a + b, (sizes[0], hex(src), hex(dst))           # the two layouts one behind the other
            assert n <= a + b + 256, (sizes[0], hex(src), hex(dst))     # ... and nothing but the alignment between them


def test_workspace_mixed_sizes_and_modes_per_image():
    auto = auto_modes(MIXED)
    assert [m & 0xFF for m in auto] == [2, 1, 6] and all(m & 0x10000 for m in auto)      # every image keeps an encoder-picked count
    fixed = [X(3), X(1), X(5)]
    for src, dst in ((fixed, auto), (fixed, X(4)), (X(2), fixed), (fixed, fixed)):
        n = need(MIXED, src, dst)
        assert n >= alone(MIXED, src) + alone(MIXED, dst) > 0
    narrow = [(64, 96), (96, 64), (67, 93)]
    assert need(narrow, MODE_RANS(4), MODE_RANS(2)) >= alone(narrow, MODE_RANS(4)) + alone(narrow, MODE_RANS(2)) > 0


def test_workspace_is_zero_for_every_refused_combination():
    same = [(96, 128)] * 3
    assert need(same, X(2), MODE_AC) > 0
    assert need(same, MODE_RANS_AUTO(3), X(2)) == 0                          # an auto mode as a source ...
    assert need(same, [X(2), MODE_RANS_AUTO(3), X(2)], X(2)) == 0            # ... of one image
    assert need(same, [X(2), MODE_RANS(4), X(2)], X(2)) == 0                 # mixed lane kinds on the source side
    assert need(same, X(2), [X(2), MODE_RANS(4, wide=1), X(2)]) == 0         # ... on the target side
    assert need(same, [MODE_AC, X(2), MODE_AC], X(2)) == 0
    assert need(MIXED, MODE_AC, X(2)) == 0                                   # the reference format with images of different sizes: source
    assert need(MIXED, X(2), MODE_AC) == 0                                   # ... target
    assert need(MIXED, X(2), X(3)) > 0
    for bad in ([(31, 128)], [(96, 8161)], [(96, 128), (16, 16)]):           # sizes outside 32 .. 8160
        assert need(bad, X(2), X(2)) == 0
    assert need(same, 0x777, X(2)) == 0 and need(same, X(2), 0x777) == 0     # unknown modes
    assert need(same, [X(2), X(2)], X(2)) == 0                               # neither one mode nor one per image
    Hs, Ws, m = _arr([96]), _arr([128]), _arr([X(2)])
    L = _lib.lib()
    assert L.llicti_transcode_workspace_bytes(None, 0, _p(Hs), _p(Ws), _p(m), 1, _p(m), 1) == 0
    assert L.llicti_transcode_workspace_bytes(None, 1, None, _p(Ws), _p(m), 1, _p(m), 1) == 0
    assert L.llicti_transcode_workspace_bytes(None, 1, _p(Hs), _p(Ws), None, 1, _p(m), 1) == 0
    assert L.llicti_transcode_workspace_bytes(None, 1, _p(Hs), _p(Ws), _p(m), 1, None, 1) == 0


def test_cli_parser_transcode():
    from llicti_amd import cli
    p = cli.build_parser()
    a = p.parse_args(["transcode", "a.llic", "b.llic", "--container", "xrans10"])
    assert (a.cmd, a.src, a.dst, a.container, a.checkpoint, a.config) == ("transcode", "a.llic", "b.llic", "xrans10", None, None)
    a = p.parse_args(["transcode", "a.llic", "b.llic", "--config", "llicti_B.json", "--checkpoint", "m.pth.tar"])
    assert a.container == "auto" and a.config == "llicti_B.json" and a.checkpoint == "m.pth.tar"
    for bad in (["transcode", "a.llic"], ["transcode", "a.llic", "b.llic", "--reduce", "1"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_host_layout_of_a_transcode(tmp_path):
    """tests/sanitize_transcode_host.cpp against llicti_amd/csrc/host_plan.hpp (g++, no HIP): the two plans' regions are disjoint, every offset
    lies inside the reported size, and the planes / CNN-output placement of the two plans agrees wherever the target's kernels read the
    decoder's buffers.  Built plain here; the file's head says how to run it under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "sanitize_transcode_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(HERE, "sanitize_transcode_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert "transcode plans ok" in out.stdout
