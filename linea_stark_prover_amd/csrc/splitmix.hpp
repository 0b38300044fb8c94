// SplitMix64, the one host generator of seeded values: lsp_seeded_setup's
// challenges and round constants (capi.cpp) and the raw columns of the
// synthetic traces (witness.cpp).  The device generator (k_gen_raw_perm) is
// counter-based and has a hash of its own.
#pragma once
#include <stdint.h>

#include "fr.hpp"

namespace lsp {

struct SplitMix64 {
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    // U4: 4 words -> 253-bit mask -> reject >= r
    Fr fr() {
        for (;;) {
            Fr c;
            for (int k = 0; k < 4; ++k) {
                const uint64_t x = next();
                c.v[2 * k] = (uint32_t)x;
                c.v[2 * k + 1] = (uint32_t)(x >> 32);
            }
            c.v[7] &= (1u << 29) - 1;
            if (fr_words_lt_mod(c)) return fr_from_canonical(c);
        }
    }
    // uniform below n: accept x < 2^64 - (2^64 mod n)
    uint64_t below(uint64_t n) {
        const unsigned __int128 two64 = (unsigned __int128)1 << 64;
        const unsigned __int128 lim = two64 - (two64 % n);
        for (;;) {
            const uint64_t x = next();
            if ((unsigned __int128)x < lim) return x % n;
        }
    }
};

}  // namespace lsp
