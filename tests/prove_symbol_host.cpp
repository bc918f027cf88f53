// prove_symbol_host.cpp -- llicti_amd/csrc/prove_symbol.hpp (the stage decoders' exact search) as a pure function on the host: every hint of small
// monotone 16-bit tables, against a linear scan that ignores the hint.  Plain g++, no HIP: tests/test_host_cpu.py builds and runs it, and
// tests/sanitize_host.sh runs it under AddressSanitizer + UBSan.
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../llicti_amd/csrc/prove_symbol.hpp"

static int ceil_log2(int v)
{
    int k = 0;
    while ((1 << k) < v) ++k;
    return k;
}

int main()
{
    const int sizes[] = { 1, 2, 3, 5, 8, 17 };           // max_symbol + 1
    long cases = 0, failures = 0;
    int worst_calls = 0;
    for (int n : sizes) {
        const int max_symbol = n - 1;
        for (int kind = 0; kind < 4; ++kind) {
            std::vector<uint32_t> e(n);
            for (int i = 0; i < n; ++i) {
                switch (kind) {
                case 0: e[i] = 3u + 1000u * (uint32_t)i; break;                    // strictly rising
                case 1: e[i] = 10u + 700u * (uint32_t)(i / 3); break;              // flat stretches
                case 2: e[i] = 65536u - (uint32_t)n + (uint32_t)i; break;          // saturated at the top: entry 0 lies above most slots
                default: e[i] = (i <= n / 2) ? 0u : 40000u; break;                 // flat at 0, then a step
                }
            }
            std::vector<uint32_t> slots = { 0u, 65535u };
            for (int i = 0; i < n; ++i) {
                slots.push_back(e[i]);
                if (e[i] > 0) slots.push_back(e[i] - 1);
                if (e[i] < 65535u) slots.push_back(e[i] + 1);
            }
            for (uint32_t slot : slots) {
                int want = 0;                                                      // the last s with s == 0 || e[s] <= slot
                for (int s = 0; s < n; ++s) if (s == 0 || e[s] <= slot) want = s;
                const uint32_t want_lo = e[want], want_hi = (want == max_symbol) ? 0x10000u : e[want + 1];
                for (int first_step = 1; first_step <= 2; ++first_step)
                    for (int hint = 0; hint <= max_symbol; ++hint) {
                        int calls = 0;
                        const llicti::Proved p = llicti::prove_symbol(
                            hint, max_symbol, first_step,
                            [&](int s1, int s2, uint32_t &eA, uint32_t &eB) { eA = e.at(s1); eB = e.at(s2); },
                            [&](int i) -> uint32_t { ++calls; return e.at(i); },
                            [&](uint32_t v) { return v <= slot; });
                        ++cases;
                        const int bound = 2 + 2 * ceil_log2(max_symbol + 2);
                        if (calls > worst_calls) worst_calls = calls;
                        if (p.lo != want || p.vlo != want_lo || p.vhi != want_hi || calls > bound) {
                            if (++failures <= 10)
                                fprintf(stderr, "n=%d kind=%d slot=%u hint=%d first_step=%d: got (%d, %u, %u) in %d calls, want (%d, %u, %u) in <= %d\n",
                                        n, kind, slot, hint, first_step, p.lo, p.vlo, p.vhi, calls, want, want_lo, want_hi, bound);
                        }
                    }
            }
        }
    }
    printf("%ld cases, %ld failures, at most %d single-entry calls\n", cases, failures, worst_calls);
    if (failures == 0) printf("clean\n");
    return failures ? 1 : 0;
}
