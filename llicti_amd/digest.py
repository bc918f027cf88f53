"""Digest manifests: the pixel digests of an archive's images in a sidecar file, `<archive>.lldg`.

A digest is zlib's CRC-32 of an image's pixels as planar uint8 [3][H][W] bytes -- `zlib.crc32(rgb_chw.tobytes())`; include/llicti_hip.h,
"PIXEL DIGESTS", defines it and the device computes it (HipCodec.digests).  The archive formats are frozen, so the digests travel beside the
archive; the manifest carries the crc32 of the archive's index, which binds it to that archive.

Layout, little-endian:

    b"LLDG", u8 version = 1, u8 algo = 1 (CRC-32 of planar RGB), u16 0, u64 count
    u32 index_crc         the archive trailer's crc32(index)
    count x u32           the digest of image k of the archive
    u32 crc32             of every byte in front of it

Every damaged field is a ValueError, and so is a count or an index crc that does not match the archive the manifest is opened for.  A digest
is a check against accidents, not a MAC.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

MAGIC = b"LLDG"
VERSION = 1
ALGO_CRC32_RGB = 1
EXT = ".lldg"
HEAD = struct.Struct("<4sBBHQI")        # magic, version, algo, zero, count, index_crc: 20 bytes


def manifest_path(archive_path) -> str:
    return str(archive_path) + EXT


def archive_index_crc(path) -> int:
    """crc32(index) as the trailer of the archive at `path` states it (.llia or .llpa: the last four bytes of the file)."""
    from .archive import TRAILER, TRAILER_BYTES
    with open(path, "rb") as fh:
        size = fh.seek(0, 2)
        if size < TRAILER_BYTES:
            raise ValueError(f"{path}: shorter than an archive trailer")
        fh.seek(size - TRAILER_BYTES)
        return int(TRAILER.unpack(fh.read(TRAILER_BYTES))[6])


def dumps_manifest(digests, index_crc) -> bytes:
    d = [int(v) for v in digests]
    if any(not 0 <= v <= 0xFFFFFFFF for v in d) or not 0 <= int(index_crc) <= 0xFFFFFFFF:
        raise ValueError("digests and the index crc are 32-bit values")
    body = HEAD.pack(MAGIC, VERSION, ALGO_CRC32_RGB, 0, len(d), int(index_crc)) + np.asarray(d, dtype="<u4").tobytes()
    return body + struct.pack("<I", zlib.crc32(body) & 0xFFFFFFFF)


def loads_manifest(data, count=None, index_crc=None, what="manifest"):
    """-> the digests, a list of ints.  count, index_crc: the opened archive's, held against the manifest's when given."""
    data = bytes(data)
    if len(data) < HEAD.size + 4:
        raise ValueError(f"{what}: shorter than a digest manifest")
    magic, version, algo, zero, n, icrc = HEAD.unpack(data[:HEAD.size])
    if magic != MAGIC:
        raise ValueError(f"{what}: not a digest manifest (bad magic)")
    if version != VERSION or zero != 0:
        raise ValueError(f"{what}: unsupported manifest version {version}")
    if algo != ALGO_CRC32_RGB:
        raise ValueError(f"{what}: unknown digest algorithm {algo}")
    if len(data) != HEAD.size + 4 * n + 4:
        raise ValueError(f"{what}: {len(data)} bytes do not hold {n} digests")
    if zlib.crc32(data[:-4]) & 0xFFFFFFFF != struct.unpack("<I", data[-4:])[0]:
        raise ValueError(f"{what}: crc32 mismatch")
    if count is not None and n != int(count):
        raise ValueError(f"{what}: {n} digests for an archive of {int(count)} images")
    if index_crc is not None and icrc != int(index_crc) & 0xFFFFFFFF:
        raise ValueError(f"{what}: written for another archive (index crc32 {icrc:08x}, this archive's is {int(index_crc) & 0xFFFFFFFF:08x})")
    return [int(v) for v in np.frombuffer(data, dtype="<u4", count=n, offset=HEAD.size)]


def write_manifest(path, digests, index_crc):
    """Write the manifest of an archive whose trailer states `index_crc` (archive_index_crc) to `path` (manifest_path(archive))."""
    data = dumps_manifest(digests, index_crc)
    with open(path, "wb") as fh:
        fh.write(data)


def read_manifest(path, archive=None):
    """-> the digests of the manifest at `path`.  archive: the opened reader (ArchiveReader / ProgressiveReader) the manifest must belong to --
    its image count and its trailer's index crc32 are held against the manifest's."""
    with open(path, "rb") as fh:
        data = fh.read()
    if archive is None:
        return loads_manifest(data, what=str(path))
    return loads_manifest(data, len(archive), archive.index_crc, what=str(path))
