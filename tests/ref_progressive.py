"""Progressive records, restated from the format text (include/llicti_hip.h "PROGRESSIVE RECORDS") -- TEST INFRASTRUCTURE, pure Python.

It shares no code with llicti_amd/progressive.py or the library: the tests hold both to this reading.  Streams are located with the second
reader of the container format (tests/ref_rans.py: parse_header), cuts are whatever the caller measured (ref_rans' cursors, or the device's).

  to_progressive(plain_record, cuts)        the .llic record of an xwide v4 container + per stream (c_1 .. c_{L-1}) -> the progressive record
  check(record, ...)                        every rule llicti_unpack_progressive states -> the parsed table, or Refused
  prefixes(record)                          [P_0 .. P_L]
  from_progressive(prefix, r, fill)         the first P_r bytes (or more) -> (payload bytes with `fill` where nothing was delivered, seg_len, mask)
  malformed_cases(record)                   one minimally edited record per rule
"""
import struct

import numpy as np

import ref_rans as rr

MODELS = {49: 5, 22: 2}


class Refused(ValueError):
    pass


def _u32s(buf, pos, k):
    return list(struct.unpack_from("<%dI" % k, buf, pos))


def locate_streams(payload, seg_len):
    """(off, len) of every stream of an xwide v4 container's payload."""
    if list(seg_len[:3]) != [3, 12, 2]:
        raise Refused("header segments")
    hdr = rr.parse_header(payload[0], payload[15] | (payload[16] << 8))
    if hdr["layout"] != "v4":
        raise Refused("not an xwide v4 container")
    M, k = hdr["M"], hdr["per_seg"]
    starts = np.concatenate(([0], np.cumsum(seg_len))).astype(np.int64)
    out = []
    for m in range(M):
        g = m // k
        s0, sn = int(starts[4 + g]), int(seg_len[4 + g])
        if k == 1:
            out.append((s0, sn))
            continue
        lens = _u32s(payload, s0, k)
        if 4 * k + sum(lens) != sn:
            raise Refused("length table")
        out.append((s0 + 4 * k + sum(lens[:m % k]), lens[m % k]))
    return hdr, out


def to_progressive(plain_record, cuts):
    """cuts[m] = (c[m][1], ..., c[m][L-1]) for every stream m of the record's container."""
    rec = bytes(plain_record)
    assert rec[:4] == b"LLIC" and rec[4] == 1
    n = rec[5]
    L = MODELS[n]
    seg_len = _u32s(rec, 6, n)
    pay = rec[6 + 4 * n:]
    assert len(pay) == sum(seg_len)
    hdr, streams = locate_streams(pay, seg_len)
    M = hdr["M"]
    assert hdr["nlevels"] == L and len(cuts) == M
    out = bytearray(b"LLIP" + bytes([1, n, L, 0]) + struct.pack("<HH", M, 0) + struct.pack("<%dI" % n, *seg_len))
    for (off, ln), c in zip(streams, cuts):
        c = [int(v) for v in c]
        assert len(c) == L - 1 and all(a <= b for a, b in zip([0] + c, c + [ln]))
        out += struct.pack("<%dI" % (L + 1), off, ln, *c)
    end = 0
    for off, ln in streams:                                        # the frame bytes: what lies between the streams
        out += pay[end:off]
        end = off + ln
    out += pay[end:]
    for l in range(L - 1, -1, -1):
        for (off, ln), c in zip(streams, cuts):
            cc = [0] + [int(v) for v in c] + [ln]
            out += pay[off + cc[l]:off + cc[l + 1]]
    return bytes(out)


def check(record, n=None, L=None, stride=None, r=None):
    """-> dict(n, L, M, seg_len, streams [(off, len, [c_0 .. c_L])], T, S, F, prefix [P_0 .. P_L]); Refused names the rule."""
    rec = bytes(record)
    if len(rec) < 12:
        raise Refused("shorter than the fixed bytes")
    if rec[:4] != b"LLIP":
        raise Refused("magic")
    if rec[4] != 1:
        raise Refused("version")
    rn, rL = rec[5], rec[6]
    if MODELS.get(rn) != rL:
        raise Refused("n / L are no model's")
    if (n is not None and rn != n) or (L is not None and rL != L):
        raise Refused("n / L are not the context's")
    if rec[7] or rec[10] or rec[11]:
        raise Refused("zero bytes")
    M = rec[8] | (rec[9] << 8)
    if not 1 <= M <= 128:
        raise Refused("M")
    T = 12 + 4 * rn + 4 * M * (rL + 1)
    if len(rec) < T:
        raise Refused("shorter than the table")
    seg_len = _u32s(rec, 12, rn)
    if any(v >= 1 << 31 for v in seg_len):
        raise Refused("segment length")
    S = sum(seg_len)
    if stride is not None and S > stride:
        raise Refused("S > stride")
    streams, end = [], 0
    for m in range(M):
        row = _u32s(rec, 12 + 4 * rn + 4 * m * (rL + 1), rL + 1)
        if any(v >= 1 << 31 for v in row):
            raise Refused("stream word")
        off, ln = row[0], row[1]
        if off < end or off + ln > S:
            raise Refused("streams ascending and disjoint inside the payload")
        c = [0] + row[2:] + [ln]
        if any(a > b for a, b in zip(c, c[1:])):
            raise Refused("cuts")
        streams.append((off, ln, c))
        end = off + ln
    F = S - sum(s[1] for s in streams)
    prefix = [T + F + sum(s[2][rL] - s[2][l] for s in streams) for l in range(rL + 1)]
    if r is not None:
        if not 0 <= r <= rL:
            raise Refused("r")
        if len(rec) < prefix[r]:
            raise Refused("shorter than P_r")
    return dict(n=rn, L=rL, M=M, seg_len=seg_len, streams=streams, T=T, S=S, F=F, prefix=prefix)


def prefixes(record):
    return check(record)["prefix"]


def from_progressive(prefix, r, fill=0xA5):
    """The first P_r bytes of a record (more are ignored) -> (payload uint8 [S], seg_len list, delivered bool [S]): the frame bytes and the
    pieces of the levels >= r at their payload positions, `fill` everywhere else."""
    t = check(prefix, r=r)
    L, S = t["L"], t["S"]
    pay = np.full(S, fill, np.uint8)
    mask = np.zeros(S, bool)
    src = np.frombuffer(bytes(prefix), np.uint8)
    pos = t["T"]
    end = 0
    for off, ln, _ in t["streams"] + [(S, 0, None)]:
        pay[end:off] = src[pos:pos + off - end]
        mask[end:off] = True
        pos += off - end
        end = off + ln
    for l in range(L - 1, r - 1, -1):
        for off, ln, c in t["streams"]:
            k = c[l + 1] - c[l]
            pay[off + c[l]:off + c[l + 1]] = src[pos:pos + k]
            mask[off + c[l]:off + c[l + 1]] = True
            pos += k
    assert pos == t["prefix"][r]
    return pay, t["seg_len"], mask


def ref_cuts(segs, rows, stop_level=0, sink=None):
    """ref_rans.decode of a container's segments with the cursors of its Stream objects read behind each level: -> (cuts, decoded) with
    cuts[m] = (cursor >> 3 behind level L-1 .. 1, listed as c_1 .. c_{L-1}).  ref_rans is not edited: Stream.__init__ is wrapped for the
    length of the call to record the instances decode() constructs, and on_stage reads them at stages 9 (L - l) - 1.
    stop_level = r >= 1: the decode is ABANDONED behind level r (the stages of a reduced decode), decoded holds the 9 (L - r) stages run."""
    made = []
    orig = rr.Stream.__init__

    def recording_init(self, *a, **k):
        orig(self, *a, **k)
        made.append(self)

    class _Stop(Exception):
        pass

    L = rr.parse_header(segs[0][0], int.from_bytes(segs[2], "little"))["nlevels"]
    at, stages = {}, []

    def on_stage(st, out):
        stages.append(out)
        if sink is not None:
            sink(st, out)
        if (st + 1) % 9 == 0:
            l = L - (st + 1) // 9
            at[l] = [s.cursor >> 3 for s in made]
            if l == stop_level and l >= 1:
                raise _Stop()

    rr.Stream.__init__ = recording_init
    try:
        rr.decode(segs, rows, on_stage=on_stage)
    except _Stop:
        pass
    finally:
        rr.Stream.__init__ = orig
    cuts = [tuple(at[l][m] for l in range(1, L) if l in at) for m in range(len(made))]
    return cuts, stages


def plain_record(segs):
    """The .llic record (fileio.dumps_llic's bytes) of a container's segments."""
    return b"LLIC" + bytes([1, len(segs)]) + struct.pack("<%dI" % len(segs), *[len(s) for s in segs]) + b"".join(bytes(s) for s in segs)


def record_segments(plain):
    rec = bytes(plain)
    n = rec[5]
    lens = _u32s(rec, 6, n)
    pos, segs = 6 + 4 * n, []
    for ln in lens:
        segs.append(rec[pos:pos + ln])
        pos += ln
    return segs


def malformed_cases(record):
    """[(name, bytes, kwargs of check that expose it)]: one minimal edit of a good record per rule.  kind "table" cases are refused from
    the table alone (llicti_progressive_prefix refuses them too); the others need the call's stride / reduce / the record's length."""
    good = bytes(record)
    t = check(good)
    n, L, M, T = t["n"], t["L"], t["M"], t["T"]
    row0 = 12 + 4 * n

    def edit(pos, fmt, val):
        b = bytearray(good)
        struct.pack_into(fmt, b, pos, val)
        return bytes(b)

    def word(m, k):
        return row0 + 4 * (m * (L + 1) + k)

    last = M - 1
    off_l, len_l, c_l = t["streams"][last]
    out = [
        ("magic", edit(3, "<B", ord("Q")), {}),
        ("version", edit(4, "<B", 2), {}),
        ("n", edit(5, "<B", n + 1), {}),
        ("L", edit(6, "<B", L + 1), {}),
        ("zero7", edit(7, "<B", 1), {}),
        ("zero10", edit(10, "<H", 0x100), {}),
        ("M=0", edit(8, "<H", 0), {}),
        ("M=129", edit(8, "<H", 129), {}),
        ("seg-2^31", edit(12 + 4 * 5, "<I", t["seg_len"][5] | 0x80000000), {}),
        ("off-2^31", edit(word(0, 0), "<I", t["streams"][0][0] | 0x80000000), {}),
        ("len-2^31", edit(word(last, 1), "<I", len_l | 0x80000000), {}),
        ("cut-2^31", edit(word(0, 2), "<I", 0x80000000), {}),
        ("past-S", edit(word(last, 1), "<I", t["S"] - off_l + 1), {}),
        ("cut>len", edit(word(last, L), "<I", len_l + 1), {}),
        ("table-cut-short", good[:T - 1], {}),
    ]
    if M >= 2:
        out.append(("overlap", edit(word(1, 0), "<I", t["streams"][1][0] - 1), {}))
    if L >= 3:
        out.append(("cuts-descend", edit(word(0, 2), "<I", t["streams"][0][2][2] + 1), {}))
    out = [(name, b, dict(kw, kind="table")) for name, b, kw in out]
    other = bytes(good[:5]) + bytes([22 if n == 49 else 49, 2 if n == 49 else 5]) + good[7:]      # (the other model's n and L: the context's rule)
    out += [
        ("other-model", other, dict(n=n, L=L, kind="call")),
        ("S>stride", good, dict(stride=t["S"] - 1, kind="call")),
        ("r>L", good, dict(r=L + 1, kind="call")),
        ("short-of-P_r", good[:t["prefix"][1] - 1], dict(r=1, kind="call")),
    ]
    return out
