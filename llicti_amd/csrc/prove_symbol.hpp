// prove_symbol.hpp -- the exact search of the rANS stage decoders: given a HINT for the symbol (from an approximate table: it may be anything), find
// the symbol s with entry[s] <= slot < entry[s + 1] using exact table entries only, so that the answer is the one an exact search of the whole row
// returns whatever the hint was.  Entry 0 is the floor of the search (torchac: left = 0), c_high of the top symbol is 0x10000 by definition.
// No HIP dependency: the pair and lane kernels of rans_coder.hpp call it on the device (the four-lane kernel keeps the same search in place:
// profiles/README.md, decoder_parts); g++ compiles tests/prove_symbol_host.cpp against it and runs it from every hint of small tables.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LLICTI_PROVE_HD __host__ __device__ __forceinline__
#else
#define LLICTI_PROVE_HD inline
#endif

namespace llicti {

struct Proved { int lo; uint32_t vlo, vhi; };        // the symbol, entry[lo], entry[lo + 1] (0x10000 at the top symbol)

// two(s1, s2, eA, eB): the entries s1 = hint and s2 = min(hint + 1, max_symbol), in whatever way the kernel evaluates two at once;
// one(i): a single entry;  le(e): "entry <= slot" as the kernel decides it (it must be uniform wherever the kernel's control flow has to be).
// The two entries the state update needs anyway are also the proof of the hint.  If it is off: gallop away from it (first_step, doubling) until
// the slot is bracketed, then bisect.
template <class Entry2, class Entry1, class Le>
LLICTI_PROVE_HD Proved prove_symbol(int hint, int max_symbol, int first_step, const Entry2 &two, const Entry1 &one, const Le &le)
{
    int lo = 0, hi = max_symbol + 1;
    uint32_t vlo = 0, vhi = 0x10000u;
    bool have_lo = false, have_hi = false;
    {
        const int s1 = hint, s2 = (hint + 1 < max_symbol) ? hint + 1 : max_symbol;
        uint32_t eA, eB;
        two(s1, s2, eA, eB);
        const bool bA = le(eA), bB = le(eB);
        const bool leA = (s1 == 0) || bA;                // entry 0 is the floor of the search
        const bool leB = (s1 + 1 <= max_symbol) && bB;   // past the top symbol: c_high = 0x10000 by definition
        if (leA) {
            lo = s1; vlo = eA; have_lo = true;
            if (leB) { lo = s2; vlo = eB; }
            else if (s1 + 1 <= max_symbol) { hi = s2; vhi = eB; have_hi = true; }
        } else { hi = s1; vhi = eA; have_hi = true; }
    }
    int step = first_step;
    while (hi - lo > 1) {
        int probe;
        if (have_lo && have_hi) probe = (lo + hi) >> 1;
        else if (have_lo) { probe = (lo + step < hi - 1) ? lo + step : hi - 1; step <<= 1; }
        else { probe = (hi - step > lo + 1) ? hi - step : lo + 1; step <<= 1; }
        const uint32_t e = one(probe);
        if (le(e)) { lo = probe; vlo = e; have_lo = true; } else { hi = probe; vhi = e; have_hi = true; }
    }
    if (!have_lo) vlo = one(0);
    return Proved{ lo, vlo, vhi };
}

}  // namespace llicti
