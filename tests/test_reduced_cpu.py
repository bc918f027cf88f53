"""Reduced-resolution decode, the parts that need no GPU: the size rule (Python and C-ABI) against numpy's own slicing, the CLI's --reduce,
the host plan of a reduced call, and the new kernel's resource usage in hipcc's device assembly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from llicti_amd import _lib
from llicti_amd.codec import reduced_dims

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _want(H, W, r):
    return np.empty((H, W), dtype=np.uint8)[::2 ** r, ::2 ** r].shape


def test_reduced_dims_equal_numpy_slicing():
    for r in range(6):
        for H in range(32, 201):
            for W in range(32, 201):
                assert reduced_dims(H, W, r) == _want(H, W, r), (H, W, r)
        for H, W in ((577, 768), (8160, 8160)):
            assert reduced_dims(H, W, r) == _want(H, W, r), (H, W, r)


def _c_dims(H, W, r):
    hr, wr = C.c_int(-1), C.c_int(-1)
    rc = _lib.lib().llicti_reduced_dims(H, W, r, C.byref(hr), C.byref(wr))
    return rc, (hr.value, wr.value)


def test_c_abi_reduced_dims_agree():
    for r in range(6):
        for H, W in [(h, w) for h in range(32, 201, 7) for w in range(32, 201)] + [(h, 77) for h in range(32, 201)] + [(577, 768), (8160, 8160)]:
            assert _c_dims(H, W, r) == (0, reduced_dims(H, W, r)), (H, W, r)


@pytest.mark.parametrize("r", [-1, 6])
def test_c_abi_reduced_dims_rejects(r):
    rc, got = _c_dims(96, 160, r)
    assert rc == _lib.EINVAL and got == (-1, -1)
    assert b"reduce" in _lib.lib().llicti_last_error()
    with pytest.raises(ValueError):
        reduced_dims(96, 160, r)


def test_cli_parser_reduce():
    from llicti_amd import cli
    p = cli.build_parser()
    a = p.parse_args(["decode", "a.llic", "b.ppm", "--reduce", "2"])
    assert a.cmd == "decode" and a.reduce == 2
    assert p.parse_args(["decode", "a.llic", "b.ppm"]).reduce == 0
    for bad in ("-1", "6", "x"):
        with pytest.raises(SystemExit):
            p.parse_args(["decode", "a.llic", "b.ppm", "--reduce", bad])


def test_cli_info_lists_the_sizes(tmp_path, capsys):
    """`info` on a reference-format container of either model (the CPU oracle writes them): one size per level the model has, r = 0 first."""
    from conftest import load_state_dict
    from helpers import make_image
    from llicti_amd import cli, fileio
    from llicti_amd.weights import pack_state_dict
    from oracle import oracle as orc
    rgb = make_image("smooth", 67, 93, 1)
    bl = orc.encode_image(rgb, orc.Weights(pack_state_dict(load_state_dict("rand1337"))))
    path = str(tmp_path / "a.llic")
    fileio.write_llic(path, bl)
    assert cli.main(["info", path]) == 0
    out = capsys.readouterr().out
    assert "r=0 93x67, r=1 47x34, r=2 24x17, r=3 12x9, r=4 6x5, r=5 3x3" in out


def test_host_plan_of_a_reduced_call(tmp_path):
    """tests/sanitize_reduced_host.cpp against llicti_amd/csrc/host_plan.hpp (g++, no HIP): the reduced plan keeps every full-size field of the
    batch's plan, its key never equals a full-size key, its table holds the sizes numpy's slicing gives.  Built plain here, like
    test_host_cpu.py::test_host_plan_logic_driver; the file's head says how to run it under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "sanitize_reduced_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(HERE, "sanitize_reduced_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert "reduced plans ok" in out.stdout


def test_unlift_reduced_kernel_has_no_scratch_and_no_spills(tmp_path):
    """hipcc's device assembly of the library (as tests/test_cnn_isa_cpu.py reads it): the new kernel's metadata says no scratch, no spilled
    registers, no LDS; it is a small streaming kernel and must stay one."""
    out = str(tmp_path / "llicti.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = [f for f in _lib.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, _lib.SOURCES[0]], stderr=subprocess.DEVNULL)
    text = open(out).read()
    blocks = [b for b in re.findall(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S) if re.search(r"\.name:\s+_Z\d+unlift_reduced_kernel", b)]
    assert len(blocks) == 1, "unlift_reduced_kernel: expected one kernel in the code object's metadata"
    f = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", blocks[0] + "\n")}
    assert f["private_segment_fixed_size"] == 0 and f["sgpr_spill_count"] == 0 and f["vgpr_spill_count"] == 0, f
    assert f["group_segment_fixed_size"] == 0 and f["agpr_count"] == 0 and f["vgpr_count"] <= 32, f
    body = re.search(r"^_Z\d+unlift_reduced_kernel\w*:.*?s_endpgm", text, re.S | re.M).group(0)
    assert "scratch_" not in body
