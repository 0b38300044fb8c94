// How the Poseidon2 launchers (k_hash.hip, k_merkle_inject.hip) shape a
// launch: the lane form a batch of n states takes, its grid, and the dispatch
// from a context's runtime (P2Layout, lanes) to a kernel's compile-time <D, LANES>.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "k_common.hpp"
#include "poseidon2.hpp"
#include "poseidon2_f29.hpp"

namespace lsp {

// a size from the environment, read by its caller once per process
inline size_t p2_env_size(const char* name, size_t dflt) {
    const char* e = std::getenv(name);
    return e ? (size_t)std::strtoull(e, nullptr, 10) : dflt;
}
// A batch of at most LSP_COOP_MAX permutations runs one state per DPP quad:
// 4 * 16384 lanes = one wave per SIMD of the 256 CUs, where the quad form's
// shorter critical path (30 vs 46 S-boxes) wins; wider batches are
// throughput-bound and keep one state per lane.
inline size_t coop_max() {
    static const size_t v = p2_env_size("LSP_COOP_MAX", 16384);
    return v;
}
// up to this many states a pair per state (2 lanes): at 32K states one wave per
// SIMD with 168 instead of 230 products on each lane's critical path
inline size_t pair_max() {
    static const size_t v = p2_env_size("LSP_PAIR_MAX", 32768);
    return v;
}
inline unsigned coop_bs() {  // 0: by width (state_grid)
    static const unsigned v = (unsigned)p2_env_size("LSP_COOP_BS", 0);
    return v;
}
inline int lanes_for(size_t n) { return n <= coop_max() ? 4 : (n <= pair_max() ? 2 : 1); }

// grid for n states: quads in 64-lane blocks (256 from 16K states: one wave
// per SIMD), pairs and single lanes in 256-lane blocks
inline void state_grid(size_t n, int lanes, unsigned& blocks, unsigned& bs) {
    // 4 lanes per state.  At 16K states (one wave per SIMD of the chip) 64-lane
    // blocks land two waves on some SIMDs (~2x the level's latency); 256-lane
    // blocks, one per CU, spread them one per SIMD.  Narrower levels: 64.
    // "At 16K" is every count above 8K: beside a host slice (host_slice.hpp) that
    // level has 16384 - (16384 >> k) states, and 64-lane blocks took its three
    // launches per 2^19 proof to about twice their time (+0.18 ms per proof in
    // the kernel trace).  Powers of two get the block size they had.
    bs = lanes == 4 ? (coop_bs() ? coop_bs() : (n > 8192 ? 256u : 64u)) : 256u;
    blocks = nblocks((size_t)lanes * n, bs);
}

// f(d), d an integral_constant of D = the S-box degree, | P2_GEN for
// caller-set linear layers (gen_lin)
template <class F>
inline void p2_dispatch(const P2Layout& L, F&& f) {
    if (L.gen_lin) {
        if (L.sbox_degree == 17)
            f(std::integral_constant<uint32_t, 17u | P2_GEN>{});
        else
            f(std::integral_constant<uint32_t, 11u | P2_GEN>{});
    } else if (L.sbox_degree == 17)
        f(std::integral_constant<uint32_t, 17u>{});
    else
        f(std::integral_constant<uint32_t, 11u>{});
}
// f(d, ln): the same, and ln an integral_constant of the lanes per state (4, 2 or 1)
template <class F>
inline void p2_dispatch(const P2Layout& L, int lanes, F&& f) {
    p2_dispatch(L, [&](auto d) {
        if (lanes == 4)
            f(d, std::integral_constant<int, 4>{});
        else if (lanes == 2)
            f(d, std::integral_constant<int, 2>{});
        else
            f(d, std::integral_constant<int, 1>{});
    });
}

}  // namespace lsp
