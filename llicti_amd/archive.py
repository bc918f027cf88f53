"""Image archives: many images in ONE `.llia` file -- their `.llic` records back to back, an index behind them.

A data set of `.llic` files is a directory of small files and a Python loop; an archive is one file whose record region is exactly the dense
blob HipCodec.pack_records writes and HipCodec.unpack_records reads, so a batch travels disk -> pinned host buffer -> device as one gather
and one copy, and is cut into containers by a kernel (`LLICTI.decode_batch_async` takes the `Batch` that `ArchiveReader.read_batch` returns).

File layout (little-endian throughout; DESIGN.md, "Image archives"):

    records   the blob: .llic records back to back from byte 0 (fileio.dumps_llic: b"LLIC", version, n, n x u32 lengths, the segments)
    index     (count + 1) x u64 record offsets (offset[count] = index_offset)
              count x { u16 H, u16 W, u32 mode }            mode: codec.mode_of_header of the record's container header
              names: count NUL-terminated UTF-8 strings
    trailer   b"LLIA", u8 version = 1, u8 n, u16 0, u64 count, u64 index_offset, u32 crc32(index)          (28 bytes, at the end of the file)

n is the segment count of every record of the archive: 49 (config A) or 22 (config B).  The index sits behind the records so that a writer
streams records without knowing their number, and a reader finds it from the fixed-size trailer.

The file layer -- RecordFileWriter, RecordFileReader -- is written once for every kind of record: a `Kind` says what tells one archive format
from another (progressive.py's `.llpa` is the second), and a subclass adds what only its records can do.
"""
from __future__ import annotations

import mmap
import struct
import zlib
from typing import NamedTuple

import numpy as np

from . import fileio
from .codec import header_dims, mode_of_header

MAGIC = b"LLIA"
VERSION = 1
TRAILER = struct.Struct("<4sBBHQQI")
TRAILER_BYTES = TRAILER.size            # 28
EXT = ".llia"


class Kind(NamedTuple):
    """An archive format, as data: the trailer's magic and version; row(n) -> the numpy dtype of a record's index row (H, W, mode, then the
    kind's own columns); min_record(n) -> the smallest legal record, bytes; parse(record bytes, n) -> the record's index row as a tuple,
    ValueError for a record that is not a well-formed one of the model of n segments."""
    magic: bytes
    version: int
    row: object
    min_record: object
    parse: object


class Batch(NamedTuple):
    """The chosen records of an archive in ONE host buffer: what LLICTI.decode_batch_async takes in place of bytestream lists.
    blob: flat uint8 host tensor (pinned on request), the records back to back; rec_off: int64 [B + 1] offsets into it; Hs, Ws, modes: per
    image, from the index; stride: the tight container stride for HipCodec.unpack_records (the largest payload rounded up to 16)."""
    blob: object
    rec_off: np.ndarray
    Hs: list
    Ws: list
    modes: list
    stride: int


def record_header_bytes(nseg) -> int:
    return 6 + 4 * int(nseg)


def parse_record(buf, nseg):
    """One .llic record (bytes-like) of an archive of `nseg` segments -> (H, W, mode) from its container header; ValueError if it is not a
    well-formed record of that model."""
    hb = record_header_bytes(nseg)
    if len(buf) < hb or bytes(buf[:4]) != fileio.MAGIC:
        raise ValueError("not an LLIC record (bad magic or shorter than its index)")
    if buf[4] != fileio.VERSION:
        raise ValueError(f"unsupported LLIC version {buf[4]}")
    if buf[5] != nseg:
        raise ValueError(f"a record of {buf[5]} segments in an archive of {nseg}")
    lens = struct.unpack("<%dI" % nseg, bytes(buf[6:hb]))
    if hb + sum(lens) != len(buf):
        raise ValueError("LLIC payload length does not match its index")
    if lens[:3] != (3, 12, 2):
        raise ValueError("malformed header segments")
    hdr = bytes(buf[hb:hb + 17])
    H, W = header_dims(hdr)
    return H, W, mode_of_header(hdr)


LLIA = Kind(MAGIC, VERSION, lambda nseg: np.dtype([("H", "<u2"), ("W", "<u2"), ("mode", "<u4")]), record_header_bytes, parse_record)


class RecordFileWriter:
    """Write an archive of KIND: append records, then close() writes index and trailer."""
    KIND: Kind

    def __init__(self, path, nseg):
        if int(nseg) not in fileio.NSEGS:
            raise ValueError(f"nseg must be one of {fileio.NSEGS} (config A, config B), got {nseg}")
        self.path, self.nseg = path, int(nseg)
        self._fh = open(path, "wb")
        self._offsets = [0]
        self._rows = []
        self._names = []

    def __len__(self):
        return len(self._rows)

    def append_records(self, blob, rec_off, names=None):
        """blob: bytes-like holding B whole records at rec_off[b] .. rec_off[b + 1] (what EncodedBatch.records gives); names: B strings or
        None (the running index as a decimal string).  The index row of each comes from the record itself (KIND.parse)."""
        if self._fh is None:
            raise ValueError("archive is closed")
        ro = np.asarray(rec_off, dtype=np.int64).reshape(-1)
        B = ro.size - 1
        if B < 0 or (names is not None and len(names) != B):
            raise ValueError("rec_off holds B + 1 offsets, names B strings")
        mv = memoryview(blob).cast("B") if not isinstance(blob, np.ndarray) else memoryview(np.ascontiguousarray(blob, dtype=np.uint8)).cast("B")
        if B and (ro[0] < 0 or (np.diff(ro) < 0).any() or ro[-1] > len(mv)):
            raise ValueError("record offsets must ascend inside the blob")
        rows = [self.KIND.parse(mv[int(ro[b]):int(ro[b + 1])], self.nseg) for b in range(B)]      # (all of them before a byte is written)
        nm = [str(len(self._rows) + b) for b in range(B)] if names is None else [str(s) for s in names]
        if any("\0" in s for s in nm):
            raise ValueError("a name holds a NUL")
        if B:
            self._fh.write(mv[int(ro[0]):int(ro[B])])          # (records b = [ro[b], ro[b + 1]) are adjacent: one write)
        base = self._offsets[-1] - (int(ro[0]) if B else 0)
        self._offsets += [base + int(v) for v in ro[1:]]
        self._rows += rows
        self._names += nm

    def _append_one(self, data, name):
        self.append_records(data, [0, len(data)], None if name is None else [name])

    def close(self):
        if self._fh is None:
            return
        index = np.asarray(self._offsets, dtype="<u8").tobytes()
        index += np.array(self._rows, dtype=self.KIND.row(self.nseg)).tobytes()
        index += b"".join(s.encode("utf-8") + b"\0" for s in self._names)
        self._fh.write(index)
        self._fh.write(TRAILER.pack(self.KIND.magic, self.KIND.version, self.nseg, 0, len(self._rows), self._offsets[-1], zlib.crc32(index) & 0xFFFFFFFF))
        self._fh.close()
        self._fh = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class RecordFileReader:
    """Memory-mapped archive of KIND.  A bad trailer (magic, version, n, offsets that do not fit the file), an index whose crc32 differs or
    whose rows a subclass refuses (_load_rows) is a ValueError; the records themselves are validated where they are used."""
    KIND: Kind

    def __init__(self, path):
        self.path = path
        what = self.KIND.magic.decode()
        self._fh = open(path, "rb")
        try:
            size = self._fh.seek(0, 2)
            if size < TRAILER_BYTES:
                raise ValueError(f"{path}: shorter than an {what} trailer")
            self._mm = mmap.mmap(self._fh.fileno(), 0, access=mmap.ACCESS_READ)
            magic, version, nseg, zero, count, index_offset, crc = TRAILER.unpack(self._mm[size - TRAILER_BYTES:size])
            if magic != self.KIND.magic:
                raise ValueError(f"{path}: not an {what} archive (bad magic)")
            if version != self.KIND.version or zero != 0:
                raise ValueError(f"{path}: unsupported {what} version {version}")
            if nseg not in fileio.NSEGS:
                raise ValueError(f"{path}: {nseg} segments per record (49 = config A, 22 = config B)")
            row = self.KIND.row(nseg)
            index_end = size - TRAILER_BYTES
            if index_offset > index_end or (count + 1) * 8 + count * (row.itemsize + 1) > index_end - index_offset:       # (offsets, a row and a NUL per image)
                raise ValueError(f"{path}: index offset {index_offset} / count {count} do not fit a file of {size} bytes")
            index = self._mm[index_offset:index_end]
            if zlib.crc32(index) & 0xFFFFFFFF != crc:
                raise ValueError(f"{path}: index crc32 mismatch")
            self.nseg, self.count, self.index_offset = int(nseg), int(count), int(index_offset)
            self.index_crc = int(crc)                          # (what a digest manifest, llicti_amd/digest.py, is bound to)
            self.offsets = np.frombuffer(index, dtype="<u8", count=count + 1).astype(np.int64)
            if self.offsets[0] != 0 or (np.diff(self.offsets) < self.KIND.min_record(nseg)).any() or self.offsets[-1] != index_offset:
                raise ValueError(f"{path}: record offsets do not tile the record region")
            rows = np.frombuffer(index, dtype=row, count=count, offset=(count + 1) * 8)
            self.sizes = [(int(h), int(w)) for h, w in zip(rows["H"], rows["W"])]
            self.modes = [int(m) for m in rows["mode"]]
            self._load_rows(rows)
            parts = index[(count + 1) * 8 + count * row.itemsize:].split(b"\0")
            if len(parts) != count + 1 or parts[-1] != b"":
                raise ValueError(f"{path}: the index does not hold {count} NUL-terminated names")
            self.names = [p.decode("utf-8") for p in parts[:-1]]
            self._u8 = np.frombuffer(self._mm, dtype=np.uint8)
        except Exception:
            self.close()
            raise

    def _load_rows(self, rows):
        """A subclass sets its own public attributes from the kind's index columns here (ValueError for a file to refuse)."""

    def __len__(self):
        return self.count

    @property
    def total_bytes(self):
        """Bytes of the record region."""
        return self.index_offset

    def _index(self, i):
        i = int(i)
        if not -self.count <= i < self.count:
            raise IndexError(i)
        return i % self.count

    def record(self, i) -> bytes:
        """The bytes of record i, whole."""
        i = self._index(i)
        return bytes(self._mm[int(self.offsets[i]):int(self.offsets[i + 1])])

    def _host_blob(self, lens, pinned):
        """Room for records of `lens` bytes back to back -> (uint8 host tensor, its numpy view, rec_off int64 [B + 1]).  pinned: page-locked
        (one asynchronous H2D copy); without a GPU runtime an ordinary buffer.  A batch hands out a VIEW blob[:n] of this tensor, not the
        tensor: measured (profiles/records_refactor/README.md), a batch whose blob is the pinned allocation itself makes the record call
        that follows its upload and decode 15-25 us slower."""
        import torch
        rec_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        blob = torch.empty((max(1, int(rec_off[-1])),), dtype=torch.uint8, pin_memory=bool(pinned and torch.cuda.is_available()))
        return blob, blob.numpy(), rec_off

    def close(self):
        self._u8 = None
        mm, self._mm = getattr(self, "_mm", None), None
        if mm is not None:
            try:
                mm.close()
            except BufferError:          # (a caller still holds a view of the mapping: it goes with the last view)
                pass
        fh, self._fh = getattr(self, "_fh", None), None
        if fh is not None:
            fh.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ArchiveWriter(RecordFileWriter):
    """Write a `.llia` archive: append records (whole blobs from the device -- HipCodec.pack_records / EncodedBatch.records() --, or single
    .llic files), then close() writes index and trailer.  H, W and mode come from each record's 17-byte container header."""
    KIND = LLIA

    def append_llic(self, data, name=None):
        """One .llic file's bytes."""
        self._append_one(data, name)


class ArchiveReader(RecordFileReader):
    """Memory-mapped `.llia` archive; its records are validated where they are used (loads_llic here, HipCodec.unpack_records on the device)."""
    KIND = LLIA

    def __getitem__(self, i):
        """-> the image's bytestream_list (fileio.loads_llic)."""
        return fileio.loads_llic(self.record(i))

    def read_batch(self, indices, pinned=True) -> Batch:
        """The records of `indices` (any order, repeats allowed) gathered into ONE host buffer -> Batch.  Each run of consecutive indices is
        one memcpy out of the mapping.  pinned: a page-locked buffer (one asynchronous H2D copy); without a GPU runtime it is an ordinary one."""
        if any(not -self.count <= int(i) < self.count for i in indices):
            raise IndexError(f"an index outside 0 .. {self.count - 1}")
        idx = [self._index(i) for i in indices]
        lens = np.array([self.offsets[i + 1] - self.offsets[i] for i in idx], dtype=np.int64)
        blob, dst, rec_off = self._host_blob(lens, pinned)
        k = 0
        while k < len(idx):
            e = k
            while e + 1 < len(idx) and idx[e + 1] == idx[e] + 1:
                e += 1
            s0, s1 = int(self.offsets[idx[k]]), int(self.offsets[idx[e] + 1])
            dst[int(rec_off[k]):int(rec_off[k]) + (s1 - s0)] = self._u8[s0:s1]
            k = e + 1
        hb = record_header_bytes(self.nseg)
        stride = max(16, (int((lens - hb).max()) + 15) // 16 * 16) if len(idx) else 16
        return Batch(blob[:max(1, int(rec_off[-1]))], rec_off, [self.sizes[i][0] for i in idx], [self.sizes[i][1] for i in idx], [self.modes[i] for i in idx], stride)


class NotAnArchive(ValueError):
    """open_archive: the file ends in no archive's trailer."""


def open_archive(path):
    """-> the reader of the archive at `path`, chosen by the magic of its trailer: ArchiveReader (`.llia`) or progressive.ProgressiveReader
    (`.llpa`); NotAnArchive (a ValueError) for a file that ends in neither, whatever that reader refuses for one that does."""
    from .progressive import ProgressiveReader
    with open(path, "rb") as fh:
        fh.seek(max(0, fh.seek(0, 2) - TRAILER_BYTES))
        tail = fh.read(TRAILER_BYTES)
    for reader in (ArchiveReader, ProgressiveReader):
        if len(tail) == TRAILER_BYTES and tail[:4] == reader.KIND.magic:
            return reader(path)
    raise NotAnArchive(f"{path}: neither an LLIA nor an LLPA archive")
