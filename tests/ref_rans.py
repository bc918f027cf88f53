"""Second, independent reading of the rANS containers ("LLICTI-rANS v3" and the 256-lane "v4") -- TEST INFRASTRUCTURE, pure Python, a DECODER.

The rANS containers are formats of this build: the reference has only torchac, so nothing outside this repository says what their bytes mean.
Until this file the only statement of them that the suite could run was oracle/llicti_oracle.c, which also wrote the frozen vectors.  This is a
second reading, written from the format TEXT alone -- the comment block "rANS containers" of oracle/llicti_oracle.h, DESIGN.md section 5 and,
for the encoder's "auto" rule, include/llicti_hip.h -- as literally as tests/ref_ac.py reads torchac: one Python int per coder state, the bit
region of a stream as ONE big int, one loop iteration per symbol and per bit field, no numpy in the coding logic.  It calls none of the oracle's
rANS entry points and shares no control flow with them.  Two readings by the same project are still not an outside reference.

What it does
  parse_header   byte 0 and the pad field's bits 10 .. 15, for every tag the text defines (config B's 0xE9 included; v2 and the retired xwide
                 v3 tags are refused)
  decode         all stages of a container, stage by stage: the CDF rows of a stage come from a callback that is handed everything decoded so
                 far, so a corrupted container is decoded the way a real reader would decode it.  The numerics are not under test here.
  every check the text names refuses the container (class Refused, .check names the check);
  every ENCODER CHOICE the decoder can see is re-derived and must match (class NotCanonical; canonical=False turns these off): the tail count
  T (v3: maximal with 32 + bits <= 31 L; v4: the first multiple of 32 whose arena reaches 7,936 bits, the share or 8,160), the v4 field
  ceil(T / 32), the one-chain / two-chain flag, and -- auto_pick -- the stream count of an "auto" container.

The plane bookkeeping at the bottom (class Planes: header geometry, where a stage's symbols go) uses numpy; it is not coding logic.
"""

M32 = 0xFFFFFFFF
TOP = 0x80000000
STATE_BITS = 31                  # a lane state is 2^31 | 31 payload bits
V3_TAIL_MAX = 2047               # 11-bit T field
V4_TAIL_MAX = 8160               # 32 * 255
V4_SPILL_MAX = 512
SEED_MAX = 31


class Refused(Exception):
    """The container violates a check the format text names.  .check is the check's short name."""

    def __init__(self, check, detail=""):
        super().__init__(f"{check}: {detail}" if detail else check)
        self.check = check


class NotCanonical(Refused):
    """The container decodes, but an encoder choice is not the one the text's rule gives."""


# ---------------------------------------------------------------------------------------------------------------- header
def parse_header(byte0, pad):
    """byte 0 of the container and its int16 pad field (as an unsigned 16-bit int) -> dict(L lanes, M streams, per_seg streams per segment,
    layout "v3" / "v4", nlevels, nflags = pad-flag bits in use)."""
    byte0 &= 0xFF
    pad &= 0xFFFF
    if not byte0 & 0x80:
        raise Refused("tag", "bit 7 clear: not a rANS container")
    if not byte0 & 0x08:
        raise Refused("tag", "bit 3 clear: format v2")
    ext = (byte0 >> 6) & 1
    v = (((byte0 >> 4) & 3) << 3) | (byte0 & 7)                # bits 5,4,2,1,0
    hi = pad >> 10
    nlevels, layout = 5, "v3"
    if not ext:
        L, M = 64, v + 1
    elif v <= 1:
        L, M = 64, 64 << v
    elif v <= 15:
        L, M = 128, v - 1
    elif v == 16 or v == 17:
        L, layout = 256, "v4"
        nlevels = 5 if v == 16 else 2
        if 1 <= hi <= 32:
            M = hi
        elif hi in (33, 34):
            M = 64 << (hi - 33)
        else:
            raise Refused("count", f"pad bits 10..15 = {hi}")
    else:
        raise Refused("tag", f"v = {v}: a retired xwide v3 tag")
    nflags = 2 * nlevels
    if layout == "v3" and hi:
        raise Refused("pad", "bits 10..15 of the pad field set outside a v4 container")
    if (pad & 0x3FF) >> nflags:
        raise Refused("pad", "pad-flag bits above the model's levels set")
    return dict(L=L, M=M, per_seg=max(1, M // 32), layout=layout, nlevels=nlevels, nflags=nflags)


def split_streams(stream_segs, hdr):
    """The M streams of a container from its 9 x nlevels stream segments.  M <= 32: one per segment, the rest empty.  64 / 128: segment g of the first
    32 holds streams g k .. g k + k - 1 (k = M / 32) behind a table of their k u32 LE lengths."""
    M, k = hdr["M"], hdr["per_seg"]
    nseg = M if k == 1 else 32
    if nseg > len(stream_segs):
        raise Refused("segments", "more streams than segments")
    for s in stream_segs[nseg:]:
        if len(s):
            raise Refused("segments", "bytes in a segment past the last stream")
    if k == 1:
        return [bytes(s) for s in stream_segs[:M]]
    out = []
    for seg in stream_segs[:32]:
        if len(seg) < 4 * k:
            raise Refused("segments", "length table cut short")
        lens = [int.from_bytes(seg[4 * i:4 * i + 4], "little") for i in range(k)]
        if 4 * k + sum(lens) != len(seg):
            raise Refused("segments", "length table does not add up to the segment")
        pos = 4 * k
        for n in lens:
            out.append(bytes(seg[pos:pos + n]))
            pos += n
    return out


# ---------------------------------------------------------------------------------------------------------------- coder
def clz32(x):
    return 32 - x.bit_length()


def floor_log2(f):
    return f.bit_length() - 1


def find_symbol(row, slot):
    """The largest s in [1, Lp - 2] with row[s] <= slot, symbol 0 if there is none: entry 0 is the floor of the search whatever it holds (it need
    not be 0, and a slot below it still means symbol 0); entry Lp - 1 is never read, the top symbol's upper bound is 0x10000."""
    top = len(row) - 2
    lo, hi = 0, top
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if row[mid] <= slot:
            lo = mid
        else:
            hi = mid - 1
    return lo


def bounds(row, s):
    c_low = row[s]
    c_high = 0x10000 if s == len(row) - 2 else row[s + 1]
    return c_low, c_high - c_low


def pop(x, row):
    """The decoder's half of x = ((x / f) << 16) + x % f + c_low: -> (symbol, f * (x >> 16) + (x & 0xFFFF) - c_low, c_low, f), the state in 32-bit
    arithmetic (a forged slot below c_low wraps; what comes out is caught, if at all, by clz <= 16 and the end-of-stream checks)."""
    slot = x & 0xFFFF
    s = find_symbol(row, slot)
    c_low, f = bounds(row, s)
    if f <= 0:
        raise Refused("slot", "empty interval")
    return s, (f * (x >> 16) + slot - c_low) & M32, c_low, f


def emit_bits(x, f):
    """The encoder's rule: the smallest n with (x >> n) < f << 16."""
    n = 0
    while (x >> n) >= (f << 16):
        n += 1
    return n


def seed_count(A):
    """n = the largest count with A^n <= 2^31, at most 31; -> (n, A^n)."""
    n, p = 0, 1
    while n < SEED_MAX and p * A <= TOP:
        p *= A
        n += 1
    return n, p


def field(big, pos, n):
    """n bits of the LSB-first region `big` from bit pos up, as an int."""
    return (big >> pos) & ((1 << n) - 1)


class Stream:
    """One stream's bytes taken apart, and the main coder's state while the stages run."""

    def __init__(self, data, L, layout):
        self.L, self.layout = L, layout
        nstate = STATE_BITS * L // 8
        if layout == "v3":
            if len(data) < 2 + nstate:
                raise Refused("length", "stream shorter than its T field and states")
            h = data[0] | (data[1] << 8)
            if h >> 14:
                raise Refused("pad", "bits 14 / 15 of the T field set")
            self.T_field, padbits = h & 0x7FF, (h >> 11) & 7
            region = data[2:len(data) - nstate]
            self.nbits = 8 * len(region) - padbits
            if self.nbits < 0:
                raise Refused("pad", "pad bits without a byte to lie in")
            self.region = int.from_bytes(region, "little")
            if self.region >> self.nbits:
                raise Refused("pad", "unused bits on top of the bit region's last byte set")
            self.cursor = self.nbits
            self.one_chain = None
        else:
            if len(data) < 2 + nstate:
                raise Refused("length", "stream shorter than its header field and states")
            region = data[:len(data) - nstate]
            if region[-1] == 0:
                raise Refused("marker", "the bit region's last byte is zero")
            top = 8 * (len(region) - 1) + region[-1].bit_length() - 1          # the end marker
            if top < 9:
                raise Refused("marker", "no room for the 9-bit field under the end marker")
            self.region = int.from_bytes(region, "little")
            f9 = field(self.region, top - 9, 9)
            self.T_field, self.one_chain = f9 & 0xFF, f9 >> 8
            self.nbits = self.cursor = top - 9
        pay = int.from_bytes(data[len(data) - nstate:], "little")
        self.x = [TOP | field(pay, STATE_BITS * l, STATE_BITS) for l in range(L)]
        self.facts = dict(layout=layout, L=L, field=self.T_field, one_chain=self.one_chain, main_bits=self.nbits)

    def renorm(self, lane):
        x = self.x[lane]
        n = clz32(x)
        if n > 16:                                               # x / f >= 2^15 after every push: a state below 2^15 was never written
            raise Refused("clz16", "a main coder state below 2^15")
        if n:
            if n > self.cursor:
                raise Refused("underrun", "the main coder reads below the bit region")
            self.cursor -= n
            x = ((x << n) | field(self.region, self.cursor, n)) & M32
        self.x[lane] = x

    def step(self, rows):
        """One step of the main coder on lanes 0 .. len(rows) - 1: first every lane's symbol, then the renormalisation lane-ascending, reading DOWN."""
        syms = []
        for lane, row in enumerate(rows):
            sym, self.x[lane], _, _ = pop(self.x[lane], row)
            syms.append(sym)
        for lane in range(len(rows)):
            self.renorm(lane)
        return syms

    def payload(self):
        p = 0
        for l in range(self.L):                                  # (every state has its leading one: built so, and restored by every renormalisation)
            p |= (self.x[l] & (TOP - 1)) << (STATE_BITS * l)
        return p


def stream_positions(nc, m, M, L):
    """Stage positions (cropped raster index n) of stream m's symbols, step by step: chunk c = m, m + M, ... holds n = c L .. c L + L - 1."""
    steps = []
    c = m
    while c * L < nc:
        steps.append(list(range(c * L, min(nc, c * L + L))))
        c += M
    return steps


def decode(segs, rows, canonical=True, on_stage=None, on_tail=None):
    """segs: the container's segments, 4 header segments then 9 x nlevels stream segments.  rows(stage, decoded) -> the stage's CDF rows, one list of
    Lp ints per symbol in cropped raster order; decoded is the list of the earlier stages' symbol lists.  -> (decoded, info).
    info: header dict, "streams": one facts dict per stream, "last_freqs": the frequencies of the last stage's symbols.
    on_tail(stream_index, j, row, slot, symbol): called for every CODED tail symbol (not the seeds' raw ones), j counting from the stream's end,
    slot = the low 16 bits of the chain's state in front of the symbol -- an observer (tests/tail_census.py); no check depends on it."""
    if len(segs[0]) != 3 or len(segs[1]) != 12 or len(segs[2]) != 2:
        raise Refused("segments", "header segment lengths")
    pad = int.from_bytes(segs[2], "little")
    hdr = parse_header(segs[0][0], pad)
    L, M, layout = hdr["L"], hdr["M"], hdr["layout"]
    nstages = 9 * hdr["nlevels"]
    if len(segs) != 4 + nstages:
        raise Refused("segments", "segment count")
    mm = [int.from_bytes(segs[1][2 * i:2 * i + 2], "little", signed=True) for i in range(6)]
    A = mm[5] - mm[2] + 1                                     # symbol values of the Cg channel
    streams = [Stream(d, L, layout) for d in split_streams(segs[4:], hdr)]
    decoded = []
    tails = None
    for st in range(nstages):
        table = rows(st, decoded)
        nc = len(table)
        out = [None] * nc
        last = st == nstages - 1
        if last:
            tails = []
        for m, s in enumerate(streams):
            steps = stream_positions(nc, m, M, L)
            seq = [n for step in steps for n in step]
            cnt = len(seq)
            T = 0
            if last:
                if layout == "v3":
                    T = s.T_field
                    if T > cnt:
                        raise Refused("T", "more tail symbols than the stream has in the last stage")
                else:
                    T = min(32 * s.T_field, cnt)
                s.facts.update(share=cnt, T=T)
                tails.append((s, seq, T))
            main = cnt - T
            q = 0
            for step in steps:
                act = step[:max(0, main - q)]
                if not act:
                    break
                for n, sym in zip(act, s.step([table[n] for n in act])):
                    out[n] = sym
                q += len(step)
        if last:
            for m, (s, seq, T) in enumerate(tails):
                note = None if on_tail is None else (lambda j, row, slot, sym, m=m: on_tail(m, j, row, slot, sym))
                if layout == "v3":
                    _tail_v3(s, seq, T, table, out, canonical, note)
                else:
                    _tail_v4(s, seq, T, table, out, A, canonical, note)
        decoded.append(out)
        if on_stage is not None:
            on_stage(st, out)
    freqs = [bounds(table[n], decoded[-1][n])[1] for n in range(len(table))]
    return decoded, dict(header=hdr, A=A, streams=[s.facts for s in streams], last_freqs=freqs)


# ---------------------------------------------------------------------------------------------------------------- tails
def _tail_v3(s, seq, T, table, out, canonical, note=None):
    """64 / 128 lanes: one chain inside the 31 L payload bits, its final state on top, the bits going down to bit 0; the first pushed symbol (the
    stream's last) started from f << 15."""
    cnt = len(seq)
    if s.cursor != 0:
        raise Refused("v3-main", f"{s.cursor} bits of the main region left unread")
    pay = s.payload()
    top = pay.bit_length()
    s.facts.update(payload_top=top)
    if T == 0:                                                  # a tail coder that pushed nothing: its start state 2^31, no bit
        if pay != TOP:
            raise Refused("v3-end-state", "a stream without a tail carries the tail coder's state 2^31 and nothing else")
        if canonical and cnt:
            raise NotCanonical("T-rule", "no tail although the stream has symbols")
        return
    if top < 32:
        raise Refused("leading-one", "no 32-bit tail state in the payload")
    cur = top - 32
    x = x_final = pay >> cur
    f = None
    for q in range(cnt - T, cnt):
        slot = x & 0xFFFF
        sym, x, _, f = pop(x, table[seq[q]])
        out[seq[q]] = sym
        if note is not None:
            note(cnt - 1 - q, table[seq[q]], slot, sym)
        if q < cnt - 1:
            n = clz32(x)
            if n > 16:
                raise Refused("clz16", "a tail coder state below 2^15")
            if n > cur:
                raise Refused("underrun", "the tail coder reads below the payload")
            cur -= n
            x = ((x << n) | field(pay, cur, n)) & M32
    if x != f << 15:
        raise Refused("v3-end-state", "the tail does not end at its start state")
    if cur != 0:
        raise Refused("v3-end-bits", f"{cur} payload bits left unread")
    if canonical and T < min(cnt, V3_TAIL_MAX):
        # T is maximal with 32 + bits <= 31 L: the symbol in front of the tail must not fit
        nxt = seq[cnt - T - 1]
        _, f2 = bounds(table[nxt], out[nxt])
        if top + emit_bits(x_final, f2) <= STATE_BITS * s.L:
            raise NotCanonical("T-rule", "one more tail symbol fits the payload")


def _tail_v4(s, seq, T, table, out, A, canonical, note=None):
    cnt = len(seq)
    L = s.L
    paybits = STATE_BITS * L
    spill = s.cursor                                            # the main decoder's cursor ends AT the spill's length
    if spill >= V4_SPILL_MAX:
        raise Refused("spill", f"{spill} bits left under the main region")
    pay = s.payload()
    arena = pay | (field(s.region, 0, spill) << paybits)
    alen = paybits + spill
    n_seed, A_n = seed_count(A)
    s.facts.update(spill=spill, A=A, n_seed=n_seed, alen=alen)
    row_of = lambda j: table[seq[cnt - 1 - j]]                 # j counts from the stream's end
    fbits = []                                                  # bits of each field, in the decoder's reading order
    if s.one_chain:                                             # (T = 0: the same form with nothing pushed -- state 0 under the marker)
        mk = arena.bit_length() - 1                             # the end marker: the arena's highest set bit
        if mk < 32:
            raise Refused("marker", "no end marker above the chain's 32-bit state")
        if spill and mk != alen - 1:
            raise Refused("marker", "a spill must end with the end marker")
        x = arena & M32
        cur = 32
        s.facts.update(tail_final_state=x)
        for j in range(T - 1, 0, -1):
            slot = x & 0xFFFF
            sym, x, _, _ = pop(x, row_of(j))
            out[seq[cnt - 1 - j]] = sym
            if note is not None:
                note(j, row_of(j), slot, sym)
            left = mk - cur
            z = clz32(x)
            if z > left:                                        # the encoder's silent start: what is left is all there is
                n = left
            elif z > 16:
                raise Refused("clz16", "a state below 2^15 with its bits still there")
            else:
                n = z
            x = ((x << n) | field(arena, cur, n)) & M32
            cur += n
            fbits.append(n)
        if cur != mk:
            raise Refused("unread", f"{mk - cur} bits left under the end marker")
        if T == 0:
            if x:
                raise Refused("final", "a chain without symbols ends at 0")
        else:
            if x >= A:
                raise Refused("final", "the chain does not end at a symbol index")
            out[seq[cnt - 1]] = x
        raw = mk + 1
    else:
        if T < 2 * n_seed:
            raise Refused("seed", "two chains need 2 n symbols")
        xa = arena & M32
        xb = arena >> (alen - 32)
        if not xa & TOP or not xb & TOP:
            raise Refused("leading-one", "a chain's final state without its leading one")
        ca, cb = 32, alen - 32
        s.facts.update(tail_final_state=xa)
        for j in range(T - 1, 2 * n_seed - 1, -1):
            slot = (xa if j % 2 == 0 else xb) & 0xFFFF
            if j % 2 == 0:
                sym, xa, _, _ = pop(xa, row_of(j))
                n = clz32(xa)
                if n > 16:
                    raise Refused("clz16", "chain A's state below 2^15")
                if ca + n > cb:
                    raise Refused("cross", "chain A reads into chain B's bits")
                xa = ((xa << n) | field(arena, ca, n)) & M32
                ca += n
            else:
                sym, xb, _, _ = pop(xb, row_of(j))
                n = clz32(xb)
                if n > 16:
                    raise Refused("clz16", "chain B's state below 2^15")
                if cb - n < ca:
                    raise Refused("cross", "chain B reads into chain A's bits")
                cb -= n
                xb = ((xb << n) | field(arena, cb, n)) & M32
            out[seq[cnt - 1 - j]] = sym
            fbits.append(n)
            if note is not None:
                note(j, row_of(j), slot, sym)
        if field(arena, ca, cb - ca):
            raise Refused("between", "set bits between the two chains")
        for x, base in ((xa, 0), (xb, n_seed)):
            seed = x - TOP
            if seed < 0 or seed >= A_n:
                raise Refused("seed", "a chain ends above A^n")
            for i in range(n_seed):
                out[seq[cnt - 1 - (base + i)]] = seed % A
                seed //= A
        raw = 64 + (ca - 32) + (alen - 32 - cb)
        s.facts.update(gap=cb - ca)
        if canonical and cb != ca and (spill or T != min(cnt, V4_TAIL_MAX)):
            raise NotCanonical("T-rule", "zeros between the chains although the tail had symbols to take")
    s.facts.update(raw_alen=raw)
    if not canonical:
        return
    # ---- the encoder's choices, re-derived
    Tmax = min(cnt, V4_TAIL_MAX)
    if s.T_field != -(-T // 32):
        raise NotCanonical("T-rule", f"field {s.T_field} for T = {T}")
    if raw < paybits and T != Tmax:
        raise NotCanonical("T-rule", "the arena is short of the payload although the tail had symbols to take")
    if T:
        Tprev = (T - 1) // 32 * 32                              # the multiple of 32 in front of T
        first = T - Tprev                                       # those symbols' fields are the first the decoder read
        if raw - sum(fbits[:first]) >= paybits and Tprev:
            raise NotCanonical("T-rule", f"the arena had reached the payload at T = {Tprev} already")
    # one chain or two: over the stream's last k <= 64 symbols, 2 n sum(16 - floor(log2 f)) >= k (64 + n), and 2 n symbols to seed with
    k = min(64, cnt)
    cost = sum(16 - floor_log2(bounds(table[seq[cnt - 1 - j]], out[seq[cnt - 1 - j]])[1]) for j in range(k))
    two = cnt >= 2 * n_seed and 2 * n_seed * cost >= k * (64 + n_seed)
    s.facts.update(two_rule=two)
    if cnt and bool(s.one_chain) == two:
        raise NotCanonical("flag-rule", f"one_chain = {s.one_chain}, the rule gives two = {two}")


def auto_pick(Mlo, freqs):
    """The encoder's "auto" count (include/llicti_hip.h, LLICTI_MODE_RANS_X_AUTO): Mlo is what the image's size gives, freqs the frequencies of the
    last stage's n symbols, S = sum(16 - floor(log2 f))."""
    n = len(freqs)
    if n == 0:
        return Mlo
    S = sum(16 - floor_log2(f) for f in freqs)
    M = Mlo
    if S >= 11 * n:
        M = min(32, Mlo + -(-Mlo // 3))
    elif S < 4 * n:
        M = -(-2 * Mlo // 3)
    if 2 * S - n < 2 * 8704 * M:                              # the last stage cannot fill M payloads with a tenth to spare
        M = Mlo if (M > Mlo and 2 * S - n >= 2 * 8704 * Mlo) else -(-Mlo // 2)
    return M


# ---------------------------------------------------------------------------------------------------------------- plane bookkeeping (not coding logic)
BAND_OFF = ((1, 1), (0, 1), (1, 0))           # band 0: x11, 1: x01, 2: x10 -- (row, column) offset inside the 2 x 2 cell


class Planes:
    """Header geometry and where a stage's symbols go: the int16 YCoCg planes (Y - 127, Co, Cg) a progressive decoder builds up.  Subclasses give
    table(lvl, band, clr, rows R, columns C, minv, maxv) -> the stage's uint16 rows; this class's rows() is the callback decode() wants."""

    def __init__(self, segs):
        import numpy as np
        self.np = np
        hdr = parse_header(segs[0][0], int.from_bytes(segs[2], "little"))
        self.nlevels = nl = hdr["nlevels"]
        pad = int.from_bytes(segs[2], "little") & ((1 << hdr["nflags"]) - 1)
        hd, wd = segs[0][1], segs[0][2]
        H, W = hd, wd
        for l in range(nl - 1, -1, -1):                        # level nl - 1 in the lowest two bits: bit 0 padW, bit 1 padH
            H, W = 2 * H - ((pad >> 1) & 1), 2 * W - (pad & 1)
            pad >>= 2
        if H < 1 or W < 1 or -(-H // (1 << nl)) != hd or -(-W // (1 << nl)) != wd:
            raise Refused("header", "pad flags contradict the coarsest grid")
        if len(segs[3]) != 3 * hd * wd:
            raise Refused("segments", "DC band length")
        self.H, self.W = H, W
        self.mm = [int.from_bytes(segs[1][2 * i:2 * i + 2], "little", signed=True) for i in range(6)]
        dc = np.frombuffer(bytes(segs[3]), np.uint8).reshape(3, hd, wd).astype(np.int32)
        R, G, B = dc
        Co = R - B
        t = B + (Co >> 1)
        Cg = G - t
        Y = t + (Cg >> 1)
        self.planes = np.zeros((3, H, W), np.int16)
        st = 1 << nl
        self.planes[:, ::st, ::st] = np.stack([Y - 127, Co, Cg]).astype(np.int16)
        self.placed = 0

    def stage(self, st):
        lvl = self.nlevels - 1 - st // 9
        return lvl, (st % 9) // 3, st % 3

    def geom(self, lvl, band):
        Hl, Wl = -(-self.H // (1 << lvl)), -(-self.W // (1 << lvl))
        oi, oj = BAND_OFF[band]
        hc = Hl // 2 if oi else (Hl + 1) // 2
        wc = Wl // 2 if oj else (Wl + 1) // 2
        np = self.np
        R = ((2 * np.arange(hc) + oi) << lvl)
        C = ((2 * np.arange(wc) + oj) << lvl)
        return hc, wc, R, C

    def limits(self, clr):
        return (-127, 128) if clr == 0 else (self.mm[clr], self.mm[3 + clr])

    def place(self, decoded):
        np = self.np
        while self.placed < len(decoded):
            lvl, band, clr = self.stage(self.placed)
            hc, wc, R, C = self.geom(lvl, band)
            v = np.array(decoded[self.placed], np.int64).reshape(hc, wc) + self.limits(clr)[0]
            self.planes[clr][np.ix_(R, C)] = v.astype(np.int16)
            self.placed += 1

    def rows(self, st, decoded):
        self.place(decoded)
        lvl, band, clr = self.stage(st)
        hc, wc, R, C = self.geom(lvl, band)
        minv, maxv = self.limits(clr)
        if maxv < minv:
            raise Refused("header", "min above max")
        t = self.table(lvl, band, clr, R, C, minv, maxv)
        Lp = maxv - minv + 2
        flat = memoryview(self.np.ascontiguousarray(t, dtype=self.np.uint16).reshape(-1))     # rows as views of Python ints, no copy
        return [flat[i * Lp:(i + 1) * Lp] for i in range(hc * wc)]


class OraclePlanes(Planes):
    """CDF rows from the CPU oracle's numerics (band_params + cdf_rows): config A only."""

    def __init__(self, segs, weights, cache=None):
        super().__init__(segs)
        self.weights = weights
        self._par = (None, None)
        self.cache = cache              # optional dict shared between decodes of near-identical containers: (stage, planes so far) -> rows

    def rows(self, st, decoded):
        if self.cache is None:
            return super().rows(st, decoded)
        import hashlib
        self.place(decoded)
        key = (st, tuple(self.mm), hashlib.blake2b(self.planes.tobytes(), digest_size=16).digest())
        if key not in self.cache:
            self.cache[key] = super().rows(st, decoded)
        return self.cache[key]

    def table(self, lvl, band, clr, R, C, minv, maxv):
        from oracle import oracle as orc
        np = self.np
        if self._par[0] != (lvl, band):
            self._par = ((lvl, band), orc.band_params(self.planes, lvl, band, self.weights))
        par = self._par[1][:len(R), :len(C)].reshape(-1, 60)
        yv = self.planes[0][np.ix_(R, C)].astype(np.float32) / np.float32(255)
        cov = self.planes[1][np.ix_(R, C)].astype(np.float32) / np.float32(255)
        return orc.cdf_rows(par, clr, yv, cov, minv, maxv)


def decode_image(segs, planes_model, canonical=True):
    """-> (int16 planes [3, H, W] -- the caller unlifts --, info)"""
    decoded, info = decode(segs, planes_model.rows, canonical=canonical)
    planes_model.place(decoded)
    return planes_model.planes, info


def segments(bl):
    """bytestream_list (rows of 9) -> flat segment list: 4 header segments, then the stream segments."""
    return list(bl[0][:4]) + [s for row in bl[1:] for s in row]
