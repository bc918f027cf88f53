/*
 * numerics_sums_host.c -- the CPU oracle's side of the exhaustive sweep of the numerics spec's scalar functions.
 * TEST INFRASTRUCTURE: plain C with its own main, linked against oracle/liboracle.so (orc_erfc is the oracle's erfc_spec).
 *
 *   gcc -O2 -std=c11 -ffp-contract=off -fno-fast-math -fopenmp tests/numerics_sums_host.c -Loracle -loracle -Wl,-rpath,<oracle> -lm
 *
 * A chunk is the 2^20 consecutive fp32 bit patterns u = c * 2^20 + k, k = 0 .. 2^20 - 1; there are 4096 of them.  Per chunk, with
 * f = orc_erfc, two sums modulo 2^64 -- S1 = sum bits(f(u)), S2 = sum (2k + 1) bits(f(u)) (the second one sees a permutation or a
 * pair of compensating errors that the first does not) -- the smallest and the largest output word, and f's error against libm's
 * double erfc:
 *   rel    largest |f(x) - erfc(x)| / erfc(x) over 0 <= x < 7, and the x it is attained at;
 *   abs    largest |f(x) - erfc(x)| over x < 0, and its x;
 *   ratio  largest error / budget over every x that is not a NaN, budget = REL erfc(|x|) + TAIL + u [x < 0], and its x
 * (REL, TAIL: tests/ref64.py's ERFC_REL and ERFC_TAIL, passed in by the caller with --budget; the defaults are 6 u and erfc(7)).
 * For the 18 chunks that meet [2, 9] the same two sums of bits(1.0f / d) over the floats d of the chunk that lie in [2, 9]: a host
 * IEEE division, compiled with the oracle's flags.
 *
 * usage: numerics_sums_host [--budget REL TAIL] all | chunks c0 c1 ... | dump c FILE
 *   all / chunks  one line per chunk on stdout:
 *                   E c S1 S2 min max rel rel_arg abs abs_arg ratio ratio_arg      (sums and words in hex, errors as C99 hex floats)
 *                   R c S1 S2                                                      (only for chunks that meet [2, 9])
 *   dump          the chunk's 2^20 output words of f, little-endian uint32, to FILE
 * The thread count is OMP_NUM_THREADS (1 if unset), never the machine's CPU count.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

float orc_erfc(float x);

#define CHUNK_BITS 20
#define CHUNK (1u << CHUNK_BITS)
#define NCHUNKS 4096
#define RECIP_LO 0x40000000u /* 2.0f */
#define RECIP_HI 0x41100000u /* 9.0f */

static inline float bits2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t f2bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

typedef struct {
    uint64_t s1, s2, r1, r2;
    uint32_t minw, maxw, rel_arg, abs_arg, ratio_arg;
    double rel, abs, ratio;
    int has_recip;
} chunk_t;

static double g_rel, g_tail;
static const double U = 0x1p-24;

static void do_chunk(uint32_t c, chunk_t *o)
{
    memset(o, 0, sizeof *o);
    o->minw = 0xFFFFFFFFu;
    const uint32_t base = c << CHUNK_BITS;
    for (uint32_t k = 0; k < CHUNK; ++k) {
        const uint32_t u = base + k;
        const float x = bits2f(u);
        const float f = orc_erfc(x);
        const uint32_t w = f2bits(f);
        o->s1 += w;
        o->s2 += (uint64_t)(2 * k + 1) * w;
        if (w < o->minw) o->minw = w;
        if (w > o->maxw) o->maxw = w;
        if (x != x) continue;                                  /* NaN: no error to speak of (the output is pinned by the sums) */
        const double xd = (double)x, ref = erfc(xd), refa = erfc(fabs(xd));
        const double err = fabs((double)f - ref);
        if (x < 0.0f) {
            if (err > o->abs) { o->abs = err; o->abs_arg = u; }
        } else if (x < 7.0f) {
            const double r = err / ref;
            if (r > o->rel) { o->rel = r; o->rel_arg = u; }
        }
        const double ratio = err / (g_rel * refa + g_tail + (x < 0.0f ? U : 0.0));
        if (ratio > o->ratio) { o->ratio = ratio; o->ratio_arg = u; }
    }
    if (base + (CHUNK - 1) >= RECIP_LO && base <= RECIP_HI) {
        o->has_recip = 1;
        for (uint32_t k = 0; k < CHUNK; ++k) {
            const uint32_t u = base + k;
            if (u < RECIP_LO || u > RECIP_HI) continue;
            const uint32_t w = f2bits(1.0f / bits2f(u));
            o->r1 += w;
            o->r2 += (uint64_t)(2 * k + 1) * w;
        }
    }
}

static int parse_chunk(const char *s, uint32_t *c)
{
    char *end;
    const unsigned long v = strtoul(s, &end, 0);
    if (*s == 0 || *end != 0 || v >= NCHUNKS) { fprintf(stderr, "bad chunk '%s' (0 .. %d)\n", s, NCHUNKS - 1); return 0; }
    *c = (uint32_t)v;
    return 1;
}

int main(int argc, char **argv)
{
    g_rel = 6.0 * U;
    g_tail = erfc(7.0);
    int a = 1;
    if (a + 2 < argc && !strcmp(argv[a], "--budget")) {
        g_rel = strtod(argv[a + 1], NULL);
        g_tail = strtod(argv[a + 2], NULL);
        a += 3;
    }
    if (a >= argc) { fprintf(stderr, "usage: %s [--budget REL TAIL] all | chunks c0 c1 ... | dump c FILE\n", argv[0]); return 2; }
    if (!strcmp(argv[a], "dump")) {
        uint32_t c;
        if (a + 3 != argc || !parse_chunk(argv[a + 1], &c)) return 2;
        uint32_t *w = malloc(sizeof(uint32_t) * CHUNK);
        if (!w) return 1;
        for (uint32_t k = 0; k < CHUNK; ++k) w[k] = f2bits(orc_erfc(bits2f((c << CHUNK_BITS) + k)));
        FILE *fo = fopen(argv[a + 2], "wb");
        if (!fo || fwrite(w, sizeof(uint32_t), CHUNK, fo) != CHUNK || fclose(fo)) { perror(argv[a + 2]); return 1; }
        free(w);
        return 0;
    }
    uint32_t n = 0;
    uint32_t *ids = malloc(sizeof(uint32_t) * NCHUNKS);
    if (!ids) return 1;
    if (!strcmp(argv[a], "all") && a + 1 == argc) {
        for (n = 0; n < NCHUNKS; ++n) ids[n] = n;
    } else if (!strcmp(argv[a], "chunks") && a + 1 < argc && argc - a - 1 <= NCHUNKS) {
        for (int i = a + 1; i < argc; ++i)
            if (!parse_chunk(argv[i], &ids[n++])) return 2;
    } else {
        fprintf(stderr, "unknown mode '%s'\n", argv[a]);
        return 2;
    }
    chunk_t *res = malloc(sizeof(chunk_t) * n);
    if (!res) return 1;
#ifdef _OPENMP
    const char *env = getenv("OMP_NUM_THREADS");
    int nt = env ? atoi(env) : 1;
    omp_set_num_threads(nt > 0 ? nt : 1);
#endif
#pragma omp parallel for schedule(dynamic, 1)
    for (uint32_t i = 0; i < n; ++i) do_chunk(ids[i], &res[i]);
    for (uint32_t i = 0; i < n; ++i) {
        const chunk_t *o = &res[i];
        printf("E %u %016llx %016llx %08x %08x %a %08x %a %08x %a %08x\n", ids[i], (unsigned long long)o->s1, (unsigned long long)o->s2,
               o->minw, o->maxw, o->rel, o->rel_arg, o->abs, o->abs_arg, o->ratio, o->ratio_arg);
        if (o->has_recip) printf("R %u %016llx %016llx\n", ids[i], (unsigned long long)o->r1, (unsigned long long)o->r2);
    }
    free(res);
    free(ids);
    return 0;
}
