"""Interleaved, pitched pixel buffers, the parts that need no GPU: the new symbols are exported and bound, the two host helpers, fileio's layout
keyword, and the host plan of a pixel call."""
import os
import re
import subprocess

import numpy as np
import pytest

from llicti_amd import _lib, fileio
from llicti_amd import codec as cd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ["llicti_pixel_bytes", "llicti_pixel_span", "llicti_encode_images_px", "llicti_decode_images_px"]


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "llicti_hip.h")).read()
    L = _lib.lib()                       # (binds every name of _SIGS: a missing export raises here)
    for name in NEW:
        assert name in _lib.EXPORTS and re.search(r"\b%s\(" % name, header), name
        assert getattr(L, name).argtypes == _lib._SIGS[name][1]
    for k, (name, v) in enumerate((("LLICTI_PIX_RGB8", cd.PIX_RGB8), ("LLICTI_PIX_BGR8", cd.PIX_BGR8), ("LLICTI_PIX_RGBA8", cd.PIX_RGBA8),
                                   ("LLICTI_PIX_BGRA8", cd.PIX_BGRA8))):
        assert v == k and re.search(r"#define %s %d\b" % (name, k), header), name
    # the argument counts the header declares
    for name in ("llicti_encode_images_px", "llicti_decode_images_px"):
        decl = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(decl.split(",")) == len(_lib._SIGS[name][1]), name


def test_pixel_bytes_and_span():
    L = _lib.lib()
    assert [L.llicti_pixel_bytes(f) for f in range(4)] == [3, 3, 4, 4]
    assert [cd.pixel_bytes(n) for n in ("rgb", "bgr", "rgba", "bgra")] == [3, 3, 4, 4] and cd.pixel_bytes("BGRA") == 4
    for bad in (-1, 4, 100):
        assert L.llicti_pixel_bytes(bad) == 0 and L.llicti_pixel_span(bad, 64, 64, 0) == 0
        with pytest.raises(ValueError):
            cd.pixel_bytes(bad)
    with pytest.raises(ValueError):
        cd.pixel_format("yuv")
    for fmt, bpp in ((0, 3), (1, 3), (2, 4), (3, 4)):
        for H, W in ((1, 1), (32, 32), (33, 35), (67, 93), (512, 768), (8160, 8160)):
            row = W * bpp
            assert L.llicti_pixel_span(fmt, H, W, 0) == H * row == cd.pixel_span(fmt, H, W)              # tight
            assert L.llicti_pixel_span(fmt, H, W, row) == H * row
            for pitch in (row + 1, (row + 255) // 256 * 256, 4 * row + 3):
                want = (H - 1) * pitch + row
                assert L.llicti_pixel_span(fmt, H, W, pitch) == want == cd.pixel_span(fmt, H, W, pitch)
                # what numpy says: the last byte of a window of an array with that row pitch
                if H * pitch < 1 << 22:
                    canvas = np.zeros((H, pitch), dtype=np.uint8)
                    win = canvas[:, :row]
                    last = win[-1:, -1:].__array_interface__["data"][0] - canvas.__array_interface__["data"][0]
                    assert want == last + 1
            for pitch in (row - 1, 1):                                                                     # shorter than a row
                if pitch < row:
                    assert L.llicti_pixel_span(fmt, H, W, pitch) == 0
                    with pytest.raises(ValueError):
                        cd.pixel_span(fmt, H, W, pitch)
        assert L.llicti_pixel_span(fmt, 0, 5, 0) == 0 and L.llicti_pixel_span(fmt, 5, 0, 0) == 0
        assert L.llicti_pixel_span(fmt, 4, 4, 1 << 31) == 0                                              # (pitches are below 2^31)


def _ppm(H, W, seed):
    hwc = np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    return hwc, b"P6\n%d %d\n255\n" % (W, H) + hwc.tobytes()


def test_fileio_layout_keyword_roundtrips_without_a_transpose(tmp_path):
    hwc, raw = _ppm(33, 35, 1)
    src = tmp_path / "a.ppm"
    src.write_bytes(raw)
    got = fileio.read_image(str(src), layout="hwc")
    assert got.dtype == np.uint8 and got.shape == (33, 35, 3) and np.array_equal(got, hwc)
    assert got.flags["C_CONTIGUOUS"] and got.base is not None                  # the file's bytes as they are: a view, nothing was shuffled
    dst = tmp_path / "b.ppm"
    fileio.write_image(str(dst), got, layout="hwc")
    assert dst.read_bytes() == raw
    # the default is what it was: planar in, planar out, the same file
    chw = fileio.read_image(str(src))
    assert chw.shape == (3, 33, 35) and np.array_equal(chw, hwc.transpose(2, 0, 1)) and chw.flags["C_CONTIGUOUS"]
    assert np.array_equal(fileio.read_image(str(src), layout="chw"), chw)
    fileio.write_image(str(tmp_path / "c.ppm"), chw)
    assert (tmp_path / "c.ppm").read_bytes() == raw
    for bad in (chw, hwc[:, :, :2], hwc.astype(np.int16)):
        with pytest.raises(ValueError):
            fileio.write_image(str(tmp_path / "d.ppm"), bad, layout="hwc")
    with pytest.raises(ValueError):
        fileio.write_image(str(tmp_path / "d.ppm"), hwc)                       # an [H, W, 3] array without the keyword is refused as before
    with pytest.raises(ValueError):
        fileio.read_image(str(src), layout="nhwc")


def test_fileio_layout_keyword_png(tmp_path):
    hwc, _ = _ppm(20, 31, 2)
    p = str(tmp_path / "a.png")
    fileio.write_image(p, hwc, layout="hwc")
    assert np.array_equal(fileio.read_image(p, layout="hwc"), hwc)
    assert np.array_equal(fileio.read_image(p), hwc.transpose(2, 0, 1))


def test_host_plan_of_a_pixel_call(tmp_path):
    """tests/sanitize_px_host.cpp against llicti_amd/csrc/host_plan.hpp (g++, no HIP): different keys for different pitches, offsets, formats and
    reduces, the planar fields of the plan unchanged, the window table right.  Built plain here; the file's head says how to run it under
    AddressSanitizer + UBSan."""
    exe = str(tmp_path / "sanitize_px_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(HERE, "sanitize_px_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert "pixel plans ok" in out.stdout
