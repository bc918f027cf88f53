"""Progressive records: the bytes of a `.llic` record in LEVEL-MAJOR order, and `.llpa` archives of them.

A rANS stream's bit region is read downwards from its end, coarse stages first, so a decode that stops after level r (`reduce = r`) has
touched only the top of every stream.  A progressive record cuts the streams of an xwide v4 container at the level boundaries and stores the
pieces coarsest level first: a decode at reduce = r needs the first P_r bytes of the record and nothing behind them -- from disk, through the
page cache and over PCIe alike.  The container does not change by a bit: `to_llic` gives the plain record back.

The record (little-endian; include/llicti_hip.h "PROGRESSIVE RECORDS").  P = the container's payload, its n segments back to back,
S bytes; stream m is P[off_m : off_m + len_m]; the payload's bytes outside every stream are the FRAME bytes (the header segments, then the
length tables of a 64- / 128-stream container).  L = the model's levels; c[m][l] = byte of stream m the main coder's cursor stands in behind
level l (HipCodec.level_cuts), c[m][0] = 0, c[m][L] = len_m; the level-l piece of stream m is its bytes [c[m][l], c[m][l + 1]).

    0        b"LLIP", u8 version = 1, u8 n (49 / 22), u8 L (5 / 2), u8 0, u16 M (1 .. 128), u16 0
    12       u32 seg_len[n]                                   the plain record's
    12+4n    per stream m: u32 off_m, u32 len_m, u32 c[m][1] .. c[m][L-1]
    T        the frame bytes, in payload order (F = S - sum len_m)                       T = 12 + 4n + 4 M (L + 1)
    T+F      the level L-1 pieces of streams 0 .. M-1, then level L-2, ..., then level 0

    P_r = T + F + sum over l >= r and m of (c[m][l+1] - c[m][l]);  P_L = T + F (the header alone: the DC band),  P_0 = T + S (everything)

A `.llpa` archive is `.llia`'s layout and file layer (archive.py) around such records: the records back to back, the index -- (count + 1) x u64 offsets,
count x { u16 H, u16 W, u32 mode, u32 P_1 .. P_L }, the names -- and the trailer b"LLPA", u8 version = 1, u8 n, u16 0, u64 count, u64
index_offset, u32 crc32(index).  `.llia` is unchanged.

Everything in this module is pure Python on the host; the device side is HipCodec.level_cuts / pack_progressive / unpack_progressive.
"""
from __future__ import annotations

import struct
from typing import NamedTuple

import numpy as np

from . import fileio
from .archive import TRAILER_BYTES, Kind, RecordFileReader, RecordFileWriter

MAGIC = b"LLIP"
VERSION = 1
FIXED = 12
MAX_STREAMS = 128
MODELS = {49: 5, 22: 2}                 # n -> L
ARCHIVE_MAGIC = b"LLPA"
ARCHIVE_VERSION = 1
EXT = ".llpa"


class Head(NamedTuple):
    """The table of a progressive record: n, L, M, the n segment lengths, per stream (off, len, (c_1 .. c_{L-1})), T, S, F and the prefix
    lengths [P_0 .. P_L]."""
    n: int
    L: int
    M: int
    seg_len: tuple
    streams: tuple
    T: int
    S: int
    F: int
    prefix: list


def table_bytes(n, L, M) -> int:
    return FIXED + 4 * n + 4 * M * (L + 1)


def parse_head(head) -> Head:
    """The first bytes of a progressive record (at least its table) -> Head; ValueError for anything llicti_unpack_progressive refuses in a
    table: magic, version, (n, L) not a model's, the zero bytes, M outside 1 .. 128, a length of 2^31 or more, streams that do not ascend
    disjointly inside the payload, cuts that do not ascend within their stream."""
    mv = memoryview(head).cast("B") if not isinstance(head, (bytes, bytearray)) else head
    if len(mv) < FIXED or bytes(mv[:4]) != MAGIC:
        raise ValueError("not a progressive record (bad magic or shorter than its fixed bytes)")
    version, n, L, z0, M, z1 = struct.unpack("<BBBBHH", bytes(mv[4:FIXED]))
    if version != VERSION:
        raise ValueError(f"unsupported progressive record version {version}")
    if MODELS.get(n) != L:
        raise ValueError(f"n = {n}, L = {L}: not a model's segment and level counts (49 / 5, 22 / 2)")
    if z0 or z1:
        raise ValueError("reserved bytes set")
    if not 1 <= M <= MAX_STREAMS:
        raise ValueError(f"{M} streams (1 .. {MAX_STREAMS})")
    T = table_bytes(n, L, M)
    if len(mv) < T:
        raise ValueError(f"{len(mv)} bytes of a table of {T}")
    words = struct.unpack("<%dI" % (n + M * (L + 1)), bytes(mv[FIXED:T]))
    if any(w >> 31 for w in words):
        raise ValueError("a length of 2^31 or more")
    seg_len, S = words[:n], sum(words[:n])
    streams, end, lvl = [], 0, [0] * L
    for m in range(M):
        row = words[n + m * (L + 1):n + (m + 1) * (L + 1)]
        off, ln, cuts = row[0], row[1], row[2:]
        if off < end or off + ln > S:
            raise ValueError(f"stream {m} overlaps its predecessor or leaves the payload")
        c = (0,) + tuple(cuts) + (ln,)
        if any(c[i] > c[i + 1] for i in range(L)):
            raise ValueError(f"the cuts of stream {m} do not ascend within it")
        for l in range(L):
            lvl[l] += c[l + 1] - c[l]
        streams.append((off, ln, tuple(cuts)))
        end = off + ln
    F = S - sum(s[1] for s in streams)
    prefix = [0] * (L + 1)
    prefix[L] = T + F
    for r in range(L - 1, -1, -1):
        prefix[r] = prefix[r + 1] + lvl[r]
    return Head(n, L, M, tuple(seg_len), tuple(streams), T, S, F, prefix)


def prefix_bytes(head) -> list:
    """[P_0 .. P_L] of the record whose first bytes (at least the table) are `head`."""
    return parse_head(head).prefix


def frame_gaps(h: Head):
    """The payload ranges outside every stream, in payload order: M + 1 of them (empty ones included)."""
    ends = [0] + [o + n for o, n, _ in h.streams]
    starts = [o for o, _, _ in h.streams] + [h.S]
    return list(zip(ends, starts))


def to_llic(record) -> bytes:
    """A whole progressive record -> the plain `.llic` record of the same container (fileio.dumps_llic's bytes)."""
    h = parse_head(record)
    if len(record) != h.prefix[0]:
        raise ValueError(f"a progressive record of {h.prefix[0]} bytes in {len(record)}")
    pay = bytearray(h.S)
    pos = h.T
    for a, b in frame_gaps(h):
        pay[a:b] = record[pos:pos + b - a]
        pos += b - a
    for l in range(h.L - 1, -1, -1):
        for off, ln, cuts in h.streams:
            c = (0,) + cuts + (ln,)
            pay[off + c[l]:off + c[l + 1]] = record[pos:pos + c[l + 1] - c[l]]
            pos += c[l + 1] - c[l]
    assert pos == len(record)
    return fileio.MAGIC + bytes([fileio.VERSION, h.n]) + struct.pack("<%dI" % h.n, *h.seg_len) + bytes(pay)


def record_meta(record):
    """(H, W, mode, Head) of a whole progressive record, from its table and the container header among its frame bytes."""
    from .codec import header_dims, mode_of_header
    h = parse_head(record)
    if len(record) != h.prefix[0]:
        raise ValueError(f"a progressive record of {h.prefix[0]} bytes in {len(record)}")
    if h.seg_len[:3] != (3, 12, 2) or h.F < 17 or (h.streams and h.streams[0][0] < 17):
        raise ValueError("malformed header segments")
    hdr = bytes(record[h.T:h.T + 17])
    H, W = header_dims(hdr)
    return H, W, mode_of_header(hdr), h


class ProgressiveBatch(NamedTuple):
    """archive.Batch's fields plus `reduce`: blob holds, back to back, exactly the prefix P_{reduce[b]} of every chosen record (rec_off: where
    each starts); stride: the tight container stride of the FULL payloads.  What LLICTI.decode_batch_async takes in place of a Batch."""
    blob: object
    rec_off: np.ndarray
    Hs: list
    Ws: list
    modes: list
    stride: int
    reduce: list


def index_row(record, nseg):
    """A whole progressive record of an archive of `nseg` segments -> its index row (H, W, mode, (P_1 .. P_L)); ValueError as record_meta's."""
    H, W, mode, h = record_meta(record)
    if h.n != nseg:
        raise ValueError(f"a record of {h.n} segments in an archive of {nseg}")
    return H, W, mode, tuple(h.prefix[1:])


LLPA = Kind(ARCHIVE_MAGIC, ARCHIVE_VERSION, lambda nseg: np.dtype([("H", "<u2"), ("W", "<u2"), ("mode", "<u4"), ("P", "<u4", (MODELS[nseg],))]),
            lambda nseg: table_bytes(nseg, MODELS[nseg], 1), index_row)


class ProgressiveWriter(RecordFileWriter):
    """Write a `.llpa` archive: append progressive records (EncodedBatch.records(progressive=True) / HipCodec.pack_progressive), close()."""
    KIND = LLPA

    def append(self, record, name=None):
        """One progressive record's bytes."""
        self._append_one(record, name)


class ProgressiveReader(RecordFileReader):
    """Memory-mapped `.llpa` archive.  A bad trailer, an index whose crc32 differs or whose prefix lengths do not descend inside their record is
    a ValueError; the records themselves are validated where they are used (to_llic here, HipCodec.unpack_progressive on the device)."""
    KIND = LLPA

    def _load_rows(self, rows):
        L = self.nlevels = MODELS[self.nseg]
        # prefix[i] = [P_0 .. P_L] of record i: P_0 is the record's length
        self.prefix = np.concatenate((np.diff(self.offsets)[:, None], rows["P"].astype(np.int64).reshape(self.count, L)), axis=1)
        if self.count and ((np.diff(self.prefix, axis=1) > 0).any() or (self.prefix[:, L] < table_bytes(self.nseg, L, 1)).any()):
            raise ValueError(f"{self.path}: prefix lengths do not descend inside their records")

    def __getitem__(self, i):
        """-> the image's bytestream_list (through to_llic: no GPU)."""
        return fileio.loads_llic(to_llic(self.record(i)))

    def payload_bytes(self, i) -> int:
        """S of record i, from its fixed bytes (P_0 - T)."""
        i = self._index(i)
        o = int(self.offsets[i])
        M = int(self._u8[o + 8]) | (int(self._u8[o + 9]) << 8)
        return int(self.prefix[i, 0]) - table_bytes(self.nseg, self.nlevels, M)

    def read_batch(self, indices, reduce=0, pinned=True) -> ProgressiveBatch:
        """The PREFIXES P_{r_b} of the records of `indices` (any order, repeats allowed; reduce: one int or one per image) gathered into ONE
        host buffer of exactly sum P_{r_b} bytes -> ProgressiveBatch.  One memcpy per image out of the mapping: nothing behind a prefix is
        touched.  pinned: a page-locked buffer (one asynchronous H2D copy); without a GPU runtime it is an ordinary one."""
        idx = [self._index(i) for i in indices]
        red = [int(r) for r in np.broadcast_to(np.asarray(reduce, dtype=np.int64), (len(idx),))]
        if any(not 0 <= r <= self.nlevels for r in red):
            raise ValueError(f"reduce outside 0 .. {self.nlevels}")
        lens = np.array([self.prefix[i, r] for i, r in zip(idx, red)], dtype=np.int64)
        blob, dst, rec_off = self._host_blob(lens, pinned)
        for k, i in enumerate(idx):
            s0 = int(self.offsets[i])
            dst[int(rec_off[k]):int(rec_off[k + 1])] = self._u8[s0:s0 + int(lens[k])]
        pay = max((self.payload_bytes(i) for i in idx), default=0)
        stride = max(16, (pay + 15) // 16 * 16)
        return ProgressiveBatch(blob[:max(1, int(rec_off[-1]))], rec_off, [self.sizes[i][0] for i in idx], [self.sizes[i][1] for i in idx], [self.modes[i] for i in idx], stride, red)
