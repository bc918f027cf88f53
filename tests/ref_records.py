"""numpy restatement of llicti_pack_records / llicti_unpack_records (include/llicti_hip.h, "RECORDS") -- what the device must write, byte for
byte, the validation verdicts and what a refused record leaves behind included -- and a second, literal reader of the `.llia` / `.llpa` archive layout
that shares no code with llicti_amd/archive.py ("Image archives").  Test infrastructure: nothing here imports the package."""
from __future__ import annotations

import struct
import zlib

import numpy as np

NSEG = 49
OK, ENOSPACE, EFORMAT = 0, -4, -5


def header_bytes(n):
    return 6 + 4 * n


def record_size(seg_row, n, stride):
    """bytes of the record of one seg_len row, 0 if the row is unusable (a negative entry, a sum above stride)"""
    row = [int(v) for v in seg_row[:n]]
    if any(v < 0 for v in row) or sum(row) > stride:
        return 0
    return header_bytes(n) + sum(row)


def pack(cont, seg_len, n, blob, blob_cap=None):
    """cont uint8 [B, stride], seg_len int32 [B, 49], blob: the uint8 array the device was handed (its content before the call) ->
    (blob after the call, rec_off int64 [B + 1], per-image status, call status)."""
    B, stride = cont.shape
    cap = len(blob) if blob_cap is None else int(blob_cap)
    out = np.array(blob, dtype=np.uint8, copy=True)
    sizes = [record_size(seg_len[b], n, stride) for b in range(B)]
    rec_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    img = np.array([OK if s else EFORMAT for s in sizes], dtype=np.int32)
    status = EFORMAT if (img != OK).any() else OK
    if rec_off[-1] > cap:
        status = ENOSPACE
    for b in range(B):
        if sizes[b] == 0 or rec_off[b + 1] > cap:
            continue
        lens = [int(v) for v in seg_len[b, :n]]
        rec = b"LLIC" + bytes([1, n]) + struct.pack("<%dI" % n, *lens) + cont[b, :sum(lens)].tobytes()
        out[rec_off[b]:rec_off[b + 1]] = np.frombuffer(rec, dtype=np.uint8)
    return out, rec_off, img, status


def check_record(blob, o0, o1, n, stride):
    """-> the record's n lengths, or None for a record the device refuses; reads nothing of the blob before the offsets are known good"""
    o0, o1, nb = int(o0), int(o1), len(blob)
    if not (0 <= o0 <= o1 <= nb) or o1 - o0 < header_bytes(n):
        return None
    rec = blob[o0:o1]
    if bytes(rec[:4]) != b"LLIC" or rec[4] != 1 or rec[5] != n:
        return None
    lens = struct.unpack("<%dI" % n, bytes(rec[6:header_bytes(n)]))
    if any(v >> 31 for v in lens):
        return None
    if header_bytes(n) + sum(lens) != o1 - o0 or sum(lens) > stride:
        return None
    return list(lens)


def unpack(blob, rec_off, n, cont, seg_len=None):
    """blob uint8 [nb], rec_off int64 [B + 1], cont: the uint8 [B, stride] array the device was handed (its content before the call) ->
    (containers after the call, seg_len int32 [B, 49], per-image status, call status)."""
    B, stride = cont.shape
    out = np.array(cont, dtype=np.uint8, copy=True)
    seg = np.zeros((B, NSEG), dtype=np.int32)
    img = np.zeros(B, dtype=np.int32)
    for b in range(B):
        lens = check_record(blob, rec_off[b], rec_off[b + 1], n, stride)
        if lens is None:
            img[b] = EFORMAT
            continue
        seg[b, :n] = lens
        p0 = int(rec_off[b]) + header_bytes(n)
        out[b, :sum(lens)] = blob[p0:p0 + sum(lens)]
    return out, seg, img, (EFORMAT if (img != OK).any() else OK)


def synthetic_containers(rng, B, n, stride, max_seg=None):
    """B containers with well-formed header segments (3, 12, 2, then arbitrary lengths) of random bytes -> (cont [B, stride], seg_len [B, 49])"""
    cont = rng.integers(0, 256, size=(B, stride), dtype=np.uint8)
    seg = np.zeros((B, NSEG), dtype=np.int32)
    for b in range(B):
        room = stride - 17
        rest = n - 3
        cap = max(1, room // rest) if max_seg is None else max_seg
        seg[b, :3] = (3, 12, 2)
        seg[b, 3:n] = rng.integers(0, cap + 1, size=rest)
        seg[b, 3 + int(rng.integers(0, rest))] = 0          # (empty segments are ordinary: a rANS container has many)
        assert seg[b].sum() <= stride
    return cont, seg


def malformed_cases(n):
    """The malformed records of the unpack tests: name -> (f, bad) with f(blob, off, stride) -> (blob, off, stride, blob_bytes) making record
    `bad` of a batch of FOUR well-formed records (blob = the four back to back, off their offsets) unusable while its three neighbours stay
    whole.  Record `bad` must hold the batch's largest payload (the stride case cuts the stride below it)."""
    other = 22 if n == 49 else 49
    hb = header_bytes(n)

    def poke(k, v):
        def f(blob, off, stride):
            blob = blob.copy()
            blob[off[1] + k] = v
            return blob, off, stride, len(blob)
        return f

    def length(delta=0, bit31=False):
        def f(blob, off, stride):
            blob = blob.copy()
            p = int(off[1]) + 6 + 4 * 4                      # segment 4: the first stream, never empty
            v = struct.unpack_from("<I", blob, p)[0]
            assert v >= 1
            struct.pack_into("<I", blob, p, (v | 0x80000000) if bit31 else v + delta)
            return blob, off, stride, len(blob)
        return f

    def short(blob, off, stride):                           # record 1 cut to 6 + 4n - 1 bytes, the others moved up behind it
        parts = [blob[off[0]:off[1]], blob[off[1]:off[1] + hb - 1], blob[off[2]:off[3]], blob[off[3]:off[4]]]
        return np.concatenate(parts), np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.int64), stride, sum(len(p) for p in parts)

    def decreasing(blob, off, stride):
        # the blob as record 2 | record 3 | record 0: offsets (l2 + l3, end, 0, l2, l2 + l3) -- record 1 = [end, 0) runs backwards, every
        # other pair bounds its own record
        r = [blob[off[k]:off[k + 1]] for k in range(4)]
        l0, l2, l3 = len(r[0]), len(r[2]), len(r[3])
        return np.concatenate((r[2], r[3], r[0])), np.array([l2 + l3, l2 + l3 + l0, 0, l2, l2 + l3], dtype=np.int64), stride, l0 + l2 + l3

    def past_end(blob, off, stride):                        # the LAST record ends one byte past the blob
        return blob, off, stride, len(blob) - 1

    def big_payload(blob, off, stride):                     # record 1's payload is one byte more than the stride
        return blob, off, int(off[2] - off[1]) - hb - 1, len(blob)

    return {"bad_magic": (poke(2, ord("X")), 1), "version_2": (poke(4, 2), 1), "n_of_the_other_config": (poke(5, other), 1),
            "length_bit_31": (length(bit31=True), 1), "sum_one_more": (length(+1), 1), "sum_one_less": (length(-1), 1),
            "shorter_than_its_header": (short, 1), "rec_off_decreasing": (decreasing, 1), "rec_off_past_the_blob": (past_end, 3),
            "payload_larger_than_stride": (big_payload, 1)}


# ---------------------------------------------------------------------------------------------- .llia and .llpa, read literally
def read_archive(buf: bytes, magic: bytes, extra_words: int):
    """An archive file's bytes -> dict(n, count, offsets, sizes, modes, extra, names, records), straight from the written layout:
         records | (count + 1) x u64 | count x (u16 H, u16 W, u32 mode, extra_words x u32) | count NUL-terminated UTF-8 names |
         magic u8 version u8 n u16 0 u64 count u64 index_offset u32 crc32(index)
    extra: per record its extra_words words (`.llpa`: P_1 .. P_L, so extra_words = L).  ValueError for anything that contradicts it."""
    if len(buf) < 28:
        raise ValueError("too short for a trailer")
    t = buf[-28:]
    if t[0:4] != magic:
        raise ValueError("magic")
    version, n = t[4], t[5]
    (zero,) = struct.unpack_from("<H", t, 6)
    count, index_offset = struct.unpack_from("<QQ", t, 8)
    (crc,) = struct.unpack_from("<I", t, 24)
    if version != 1 or zero != 0:
        raise ValueError("version")
    if n not in (49, 22):
        raise ValueError("n")
    end = len(buf) - 28
    if index_offset > end:
        raise ValueError("index offset past the file")
    index = buf[index_offset:end]
    if zlib.crc32(index) & 0xFFFFFFFF != crc:
        raise ValueError("crc")
    per = 8 + 4 * extra_words
    if len(index) < (count + 1) * 8 + count * per:
        raise ValueError("index too short")
    offsets = [struct.unpack_from("<Q", index, 8 * k)[0] for k in range(count + 1)]
    pos = (count + 1) * 8
    sizes, modes, extra = [], [], []
    for k in range(count):
        H, W, mode = struct.unpack_from("<HHI", index, pos + per * k)
        sizes.append((H, W))
        modes.append(mode)
        extra.append(list(struct.unpack_from("<%dI" % extra_words, index, pos + per * k + 8)))
    pos += per * count
    names = []
    for k in range(count):
        e = index.index(b"\0", pos)
        names.append(index[pos:e].decode("utf-8"))
        pos = e + 1
    if pos != len(index):
        raise ValueError("bytes behind the names")
    if offsets[0] != 0 or offsets[-1] != index_offset or any(a > b for a, b in zip(offsets, offsets[1:])):
        raise ValueError("offsets")
    return dict(n=n, count=count, offsets=offsets, sizes=sizes, modes=modes, extra=extra, names=names,
                records=[buf[offsets[k]:offsets[k + 1]] for k in range(count)])


def read_llia(buf: bytes):
    """A `.llia` file's bytes, read literally: read_archive with its magic and no extra index words."""
    return read_archive(buf, b"LLIA", 0)
