"""Pixel digests without a GPU: the host arithmetic (llicti_crc32_combine against zlib, the kernel's geometry), the digest manifest
(llicti_amd/digest.py: round trip, every damaged field refused, a manifest of another archive refused), the command line's new flags and
`verify`, and the C-ABI's symbols.  Every reference is zlib."""
import ctypes as C
import os
import re
import struct
import zlib

import numpy as np
import pytest

from conftest import ROOT

LENGTHS = [0, 1, 3, 4, 255, 256, 65537]


def _bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def test_symbols_present_and_bound():
    from llicti_amd import _lib
    _lib.build()
    header = open(os.path.join(ROOT, "include", "llicti_hip.h")).read()
    assert "PIXEL DIGESTS" in header
    L = _lib.lib()                       # (binds every name of _SIGS: a missing export raises here)
    raw = C.CDLL(_lib.SO_PATH)
    for name in ("llicti_crc32_combine", "llicti_crc32_geometry", "llicti_crc32_planes", "llicti_digest_images"):
        assert name in _lib.EXPORTS and hasattr(raw, name), name
        decl = re.search(r"\b%s\(([^;]*)\);" % name, header).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl).split(",")) == len(_lib._SIGS[name][1]) == len(getattr(L, name).argtypes), name
    assert _lib._SIGS["llicti_crc32_combine"][0] is C.c_uint32


@pytest.mark.parametrize("la", LENGTHS)
def test_combine_against_zlib(la):
    from llicti_amd.codec import crc32_combine
    a = _bytes(la, 100 + la)
    for lb in LENGTHS:
        b = _bytes(lb, 7000 + lb)
        assert crc32_combine(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b), (la, lb)


def test_combine_length_above_32_bits():
    """len_b = 2^32 + 5 against chained combines of smaller pieces: B's own CRC is arbitrary, only its length enters A's shift"""
    from llicti_amd.codec import crc32_combine
    ca, ct = zlib.crc32(b"the front part"), zlib.crc32(_bytes(5, 3))
    # crc32 of 2^31 zero bytes by doubling, Z(2 n) = combine(Z(n), Z(n), n), from zlib's own value for 2^16 (the first step against zlib too)
    z, n = zlib.crc32(bytes(1 << 16)), 1 << 16
    assert crc32_combine(z, z, n) == zlib.crc32(bytes(1 << 17))
    while n < (1 << 31):
        z, n = crc32_combine(z, z, n), 2 * n
    # B = 2^32 zero bytes, then 5 bytes.  A || B in pieces of at most 2^31 bytes ...
    chained = crc32_combine(crc32_combine(crc32_combine(ca, z, 1 << 31), z, 1 << 31), ct, 5)
    # ... against ONE combine with crc32(B), itself made of pieces of at most 2^31 bytes, and B's length of 2^32 + 5
    cb = crc32_combine(crc32_combine(z, z, 1 << 31), ct, 5)
    assert crc32_combine(ca, cb, (1 << 32) + 5) == chained
    assert crc32_combine(ca, cb, 5) != chained                   # (the length's high word is not dropped)


def test_combine_associative_over_the_three_planes():
    from helpers import make_image
    from llicti_amd.codec import crc32_combine
    rgb = make_image("noise", 67, 93, 5)
    n = 67 * 93
    r, g, b = (zlib.crc32(rgb[c].tobytes()) for c in range(3))
    left = crc32_combine(crc32_combine(r, g, n), b, n)
    right = crc32_combine(r, crc32_combine(g, b, n), 2 * n)
    assert left == right == zlib.crc32(rgb.tobytes())


def test_geometry():
    from llicti_amd.codec import crc32_geometry
    lane, group = crc32_geometry()
    assert lane > 0 and group > 0 and group % lane == 0
    assert 2 * group + lane + 3 <= 8160 * 8160


# ------------------------------------------------------------------------------------------------ manifest
def _archive(path, n=3, seed=0):
    """a small .llia archive of n fake-but-well-formed records is more than these tests need: the manifest binds to the TRAILER's index crc"""
    from llicti_amd import archive
    index = _bytes(40 + seed, seed)
    with open(path, "wb") as fh:
        fh.write(index)
        fh.write(archive.TRAILER.pack(archive.MAGIC, archive.VERSION, 49, 0, n, 0, zlib.crc32(index) & 0xFFFFFFFF))
    return zlib.crc32(index) & 0xFFFFFFFF


class _Reader:
    def __init__(self, count, index_crc):
        self.count, self.index_crc = count, index_crc

    def __len__(self):
        return self.count


def test_manifest_round_trip(tmp_path):
    from llicti_amd import digest
    arc = str(tmp_path / "a.llia")
    icrc = _archive(arc)
    assert digest.archive_index_crc(arc) == icrc
    crcs = [0, 0xFFFFFFFF, 0x12345678]
    path = digest.manifest_path(arc)
    assert path == arc + ".lldg"
    digest.write_manifest(path, crcs, icrc)
    data = open(path, "rb").read()
    assert len(data) == 20 + 4 * 3 + 4 and data[:4] == b"LLDG" and data[4:8] == bytes([1, 1, 0, 0])
    assert struct.unpack("<QI", data[8:20]) == (3, icrc)
    assert digest.read_manifest(path) == crcs
    assert digest.read_manifest(path, _Reader(3, icrc)) == crcs
    digest.write_manifest(path, [], icrc)
    assert digest.read_manifest(path, _Reader(0, icrc)) == []
    with pytest.raises(ValueError):
        digest.dumps_manifest([1 << 32], icrc)


def _refresh(data):
    return data[:-4] + struct.pack("<I", zlib.crc32(data[:-4]) & 0xFFFFFFFF)


def test_manifest_every_damaged_field_refused(tmp_path):
    from llicti_amd import digest
    icrc = 0xCAFEF00D
    good = digest.dumps_manifest([11, 22, 33], icrc)
    rd = _Reader(3, icrc)
    assert digest.loads_manifest(good, 3, icrc) == [11, 22, 33]
    # any single flipped bit is refused: by the field's own check or by the manifest's crc32
    for bit in range(8 * len(good)):
        bad = bytearray(good)
        bad[bit >> 3] ^= 1 << (bit & 7)
        with pytest.raises(ValueError):
            digest.loads_manifest(bytes(bad), 3, icrc)
    # every header field, damaged under a REFRESHED crc32: the field's own check
    fields = {"magic": (0, b"LLDH"), "version": (4, b"\x02"), "algo": (5, b"\x02"), "zero": (6, b"\x01\x00"), "count": (8, struct.pack("<Q", 2)),
              "count_large": (8, struct.pack("<Q", 1 << 40)), "index_crc": (16, struct.pack("<I", icrc ^ 1))}
    for name, (off, val) in fields.items():
        bad = bytearray(good)
        bad[off:off + len(val)] = val
        with pytest.raises(ValueError):
            digest.loads_manifest(_refresh(bytes(bad)), rd.count, rd.index_crc, what=name)
    # truncated, extended
    for bad in (good[:-1], good + b"\0", good[:10], b""):
        with pytest.raises(ValueError):
            digest.loads_manifest(bad, 3, icrc)
    # a digest changed under a refreshed crc32 is a different manifest, not a damaged one
    other = bytearray(good)
    other[20] ^= 1
    assert digest.loads_manifest(_refresh(bytes(other)), 3, icrc) == [10, 22, 33]


def test_manifest_of_another_archive_refused(tmp_path):
    from llicti_amd import digest
    a, b = str(tmp_path / "a.llia"), str(tmp_path / "b.llia")
    ia, ib = _archive(a, 3, seed=1), _archive(b, 3, seed=2)
    assert ia != ib
    digest.write_manifest(digest.manifest_path(a), [1, 2, 3], ia)
    assert digest.read_manifest(digest.manifest_path(a), _Reader(3, ia)) == [1, 2, 3]
    with pytest.raises(ValueError, match="another archive"):
        digest.read_manifest(digest.manifest_path(a), _Reader(3, ib))
    with pytest.raises(ValueError, match="4 images"):
        digest.read_manifest(digest.manifest_path(a), _Reader(4, ia))


def test_reader_exposes_the_index_crc(tmp_path):
    """a real (empty) archive: the reader's index_crc is the trailer's, which is what the manifest stores"""
    from llicti_amd import archive, digest
    path = str(tmp_path / "e.llia")
    archive.ArchiveWriter(path, 49).close()
    with archive.ArchiveReader(path) as ar:
        assert len(ar) == 0 and ar.index_crc == digest.archive_index_crc(path)
        digest.write_manifest(digest.manifest_path(path), [], ar.index_crc)
        assert digest.read_manifest(digest.manifest_path(path), ar) == []


# ------------------------------------------------------------------------------------------------ command line
def test_cli_parsers():
    from llicti_amd import cli
    ap = cli.build_parser()
    a = ap.parse_args(["verify", "set.llia"])
    assert (a.cmd, a.archive, a.batch, a.config, a.checkpoint) == ("verify", "set.llia", 24, None, None)
    a = ap.parse_args(["verify", "set.llpa", "--batch", "3", "--config", "b.json", "--checkpoint", "m.pth.tar"])
    assert (a.batch, a.config, a.checkpoint) == (3, "b.json", "m.pth.tar")
    assert ap.parse_args(["pack", "a.llia", "x.png", "--digests"]).digests is True
    assert ap.parse_args(["pack", "a.llia", "x.png"]).digests is False
    assert ap.parse_args(["encode", "x.png", "x.llic", "--digest"]).digest is True
    assert ap.parse_args(["encode", "x.png", "x.llic"]).digest is False
    assert ap.parse_args(["decode", "x.llic", "x.png", "--crc32", "DEADbeef"]).crc32 == 0xDEADBEEF
    assert ap.parse_args(["decode", "x.llic", "x.png"]).crc32 is None
    for bad in (["decode", "a", "b", "--crc32", "xyz"], ["decode", "a", "b", "--crc32", "123456789"], ["verify"], ["verify", "a", "--batch", "0"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    # the existing parsers keep their arguments and defaults
    p = ap.parse_args(["pack", "a.llia", "x.png"])
    assert (p.container, p.batch, p.progressive, p.checkpoint, p.config) == ("ac", 24, False, None, None)
    d = ap.parse_args(["decode", "a", "b"])
    assert (d.reduce, d.checkpoint, d.config) == (0, None, None)


def test_cli_digest_flags_refuse_what_they_cannot_do(tmp_path, capsys):
    from llicti_amd import cli
    llic = tmp_path / "x.llic"
    llic.write_bytes(b"LLIC\x011" + bytes(4 * 49))
    assert cli.main(["pack", str(tmp_path / "a.llia"), str(llic), "--digests"]) == 2
    assert "pixels are not at hand" in capsys.readouterr().err
    assert cli.main(["decode", str(llic), str(tmp_path / "x.ppm"), "--crc32", "0", "--reduce", "1"]) == 2


def test_the_kernels_fold_on_the_host_under_sanitizers(tmp_path):
    """tests/sanitize_digest_host.cpp (a program of its own; g++, no HIP) replays the two kernels' fold with llicti_amd/csrc/crc_math.hpp -- the
    tables a context uploads, a lane's and a group's constant, the ragged end in front, the planes' fold, zlib's complements -- at the kernel's
    seams, against a bytewise CRC-32, under AddressSanitizer and UBSan."""
    import subprocess
    exe = str(tmp_path / "sanitize_digest_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize_digest_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "digest fold ok: 15 sizes" in out.stdout, (out.stdout + out.stderr)[-2000:]
