// progressive.hpp -- the progressive record ("LLIP", include/llicti_hip.h: PROGRESSIVE RECORDS): what its table must satisfy and the prefix
// arithmetic, ONCE, for the device check (records_progressive.hpp: prog_check_kernel), the two copy kernels and the host helper
// llicti_progressive_prefix.  Plain C++17 with no HIP dependency, like host_types.hpp: g++ compiles it under AddressSanitizer / UBSan
// (tests/sanitize_progressive_host.cpp).
//
//   0        b"LLIP", u8 version = 1, u8 n (49 / 22), u8 L (5 / 2), u8 0, u16 M (1 .. 128), u16 0
//   12       u32 seg_len[n]                                   the plain record's
//   12+4n    per stream m: u32 off_m, u32 len_m, u32 c[m][1] .. c[m][L-1]                          (L + 1 words a stream)
//   T        the frame bytes -- the payload's bytes outside every stream --, in payload order      T = 12 + 4n + 4 M (L + 1)
//   T+F      the level L-1 pieces of streams 0 .. M-1, then level L-2, ..., then level 0           piece (m, l) = stream bytes [c[m][l], c[m][l+1])
// with c[m][0] = 0 and c[m][L] = len_m.  Every function below reads the record's bytes one by one: a record sits at any byte offset.
#pragma once
#include "host_types.hpp"

constexpr int kProgVersion = 1;
constexpr int kProgFixed = 12;
constexpr int kProgMaxStreams = 128;
constexpr int kProgMaxPieces = kProgMaxStreams + 1 + kProgMaxStreams * LLICTI_NLEVELS;      // 769: the M + 1 frame gaps, then L pieces a stream

LLICTI_HD uint32_t prog_u32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
LLICTI_HD long prog_table_bytes(int n, int L, int M) { return kProgFixed + 4L * n + 4L * M * (L + 1); }

struct ProgHead { int n, L, M; long T; };

// The 12 fixed bytes of a record of which `bytes` are present: magic, version, (n, L) one of the two models' -- and the caller's, unless n_want
// is 0 --, the zero bytes, 1 <= M <= 128, and room for the whole table.  Reads rec[0 .. 11] alone, and only if they are present.
LLICTI_HD bool prog_head(const uint8_t *rec, long bytes, int n_want, int L_want, ProgHead *h)
{
    if (bytes < kProgFixed) return false;
    if (rec[0] != 'L' || rec[1] != 'L' || rec[2] != 'I' || rec[3] != 'P' || rec[4] != kProgVersion) return false;
    const int n = rec[5], L = rec[6], M = (int)rec[8] | ((int)rec[9] << 8);
    if (rec[7] != 0 || rec[10] != 0 || rec[11] != 0) return false;
    if (!((n == LLICTI_NSEG && L == LLICTI_NLEVELS) || (n == 22 && L == 2))) return false;
    if (n_want != 0 && (n != n_want || L != L_want)) return false;
    if (M < 1 || M > kProgMaxStreams) return false;
    h->n = n; h->L = L; h->M = M; h->T = prog_table_bytes(n, L, M);
    return bytes >= h->T;
}

// segment k's length: below 2^31
LLICTI_HD bool prog_seg(const uint8_t *rec, int k, long *v)
{
    const uint32_t u = prog_u32(rec + kProgFixed + 4 * k);
    *v = (long)u;
    return (u >> 31) == 0;
}

LLICTI_HD const uint8_t *prog_row(const uint8_t *rec, const ProgHead &h, int m) { return rec + kProgFixed + 4L * h.n + 4L * m * (h.L + 1); }

// Stream m's row against a payload of S bytes: every word below 2^31, the stream at or behind the end of stream m - 1 (whose row is read again
// here, so that the streams can be checked independently of each other) and inside [0, S), 0 <= c[1] <= ... <= c[L-1] <= len.
// -> off, len and the L piece lengths, piece[l] = c[l + 1] - c[l].
LLICTI_HD bool prog_stream(const uint8_t *rec, const ProgHead &h, int m, long S, long *off, long *len, long *piece)
{
    const uint8_t *row = prog_row(rec, h, m);
    const uint32_t o = prog_u32(row), n = prog_u32(row + 4);
    if ((o >> 31) || (n >> 31)) return false;
    long prev_end = 0;
    if (m > 0) {
        const uint8_t *prow = prog_row(rec, h, m - 1);
        const uint32_t po = prog_u32(prow), pn = prog_u32(prow + 4);
        if ((po >> 31) || (pn >> 31)) return false;
        prev_end = (long)po + (long)pn;
    }
    if ((long)o < prev_end || (long)o + (long)n > S) return false;
    // (every loop over the levels has LLICTI_NLEVELS trips and constant indices: on the device `piece` stays in registers)
    long c = 0;
    bool ok = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int l = 0; l < LLICTI_NLEVELS; ++l) {
        long next = (long)n;
        if (l + 1 < h.L) {
            const uint32_t v = prog_u32(row + 8 + 4 * l);      // c[l + 1]
            if ((v >> 31) || (long)v < c || v > n) ok = false;
            next = (long)v;
        }
        piece[l] = l < h.L ? next - c : 0;
        c = next;
    }
    *off = (long)o; *len = (long)n;
    return ok;
}

// P_r = T + F + sum over l >= r of the level's pieces, r = 0 .. L (P_L: the table and the frame bytes; P_0 = T + S); entries above L are 0.
// used: the sum of the stream lengths, lvl[l]: the sum of the level-l pieces.
LLICTI_HD void prog_prefixes(const ProgHead &h, long S, long used, const long *lvl, int64_t *prefix)
{
    long p = h.T + (S - used);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = LLICTI_NLEVELS; r >= 0; --r) {
        if (r < h.L) p += lvl[r < LLICTI_NLEVELS ? r : 0];
        prefix[r] = r > h.L ? 0 : p;
    }
}
// entry r of a prefix table, r = 0 .. LLICTI_NLEVELS (on the device: without indexing the table by a variable)
LLICTI_HD int64_t prog_prefix_at(const int64_t *prefix, int r)
{
    int64_t v = prefix[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 1; k <= LLICTI_NLEVELS; ++k) if (k == r) v = prefix[k];
    return v;
}

// The whole check, one stream after the other (the host's form; prog_check_kernel runs the same functions with a thread per segment and per
// stream).  stride < 0: no limit on S.  -> the head and prefix[0 .. LLICTI_NLEVELS].
LLICTI_HD bool prog_check(const uint8_t *rec, long bytes, int n_want, int L_want, long stride, ProgHead *h, int64_t *prefix)
{
    if (!prog_head(rec, bytes, n_want, L_want, h)) return false;
    long S = 0;
    for (int k = 0; k < h->n; ++k) {
        long v;
        if (!prog_seg(rec, k, &v)) return false;
        S += v;
    }
    if (stride >= 0 && S > stride) return false;
    long lvl[LLICTI_NLEVELS] = { 0, 0, 0, 0, 0 }, used = 0;
    for (int m = 0; m < h->M; ++m) {
        long off, len, piece[LLICTI_NLEVELS];
        if (!prog_stream(rec, *h, m, S, &off, &len, piece)) return false;
        used += len;
        for (int l = 0; l < LLICTI_NLEVELS; ++l) lvl[l] += piece[l];
    }
    prog_prefixes(*h, S, used, lvl, prefix);
    return true;
}

// Piece i of a VALIDATED record in the order of its dense side: i = 0 .. M are the frame gaps ([end of stream i - 1, start of stream i), the
// payload's start and end S at the two ends), i = M + 1 + j M + m the level L - 1 - j piece of stream m.  -> where it lies in the payload.
LLICTI_HD void prog_piece(const uint8_t *rec, const ProgHead &h, long S, int i, long *pay, long *len)
{
    if (i <= h.M) {
        long a = 0, b = S;
        if (i > 0) { const uint8_t *row = prog_row(rec, h, i - 1); a = (long)prog_u32(row) + (long)prog_u32(row + 4); }
        if (i < h.M) b = (long)prog_u32(prog_row(rec, h, i));
        *pay = a; *len = b - a;
        return;
    }
    const int k = i - (h.M + 1), l = h.L - 1 - k / h.M, m = k % h.M;
    const uint8_t *row = prog_row(rec, h, m);
    const long c0 = l == 0 ? 0 : (long)prog_u32(row + 4 + 4 * l), c1 = l == h.L - 1 ? (long)prog_u32(row + 4) : (long)prog_u32(row + 8 + 4 * l);
    *pay = (long)prog_u32(row) + c0; *len = c1 - c0;
}
LLICTI_HD int prog_piece_count(const ProgHead &h, int r) { return h.M + 1 + (h.L - r) * h.M; }      // pieces of the prefix P_r
