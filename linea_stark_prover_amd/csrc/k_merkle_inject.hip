// The injecting level of a mixed-height Merkle tree (p3-merkle-tree's
// compress_and_inject): where a class of shorter
// matrices has as many rows as the level has nodes,
//   dst[i] = compress(compress(src[2i], src[2i+1]), inj[i]),
// inj[i] = the sponge digest of row i of the class (launch_hash_rows).
//
// A translation unit of its own, so that adding it left k_hash.hip's kernels
// as compiled before (profiles/mixed_mmcs_codegen.txt).  The launcher restates
// k_hash.hip's lanes_for / state_grid thresholds, knobs included: an injecting
// level takes the lane form a plain level of its width takes.
#include <cstdlib>

#include "k_common.hpp"
#include "kernels.hpp"
#include "poseidon2_f29.hpp"

namespace lsp {

namespace {
// LANES: lanes per node -- 4 (a DPP quad), 2 (a pair) or 1, as in k_merkle_level.
// The first compression's digest goes into the second as a canonical ark-form
// word, the form every digest in memory has: no operand of the second
// permutation is outside the bounds tests/test_f29_bounds.py models.
// inj may be dst itself: a node's lanes read inj[i] before the first
// permutation and its lead lane alone writes dst[i], after the second.
template <uint32_t D, int LANES>
__global__ __launch_bounds__(256) void k_merkle_inject(const Fr* __restrict__ src, const Fr* inj, Fr* dst, size_t nout,
                                                       const F29* __restrict__ rc, uint32_t rf, uint32_t rp) {
    // the narrow forms are two permutations' latency per level, the critical path
    if constexpr (LANES > 1) __builtin_amdgcn_s_setprio(3);
    __shared__ uint4 qt[3 * F29_QTAB_N];  // f29_reduce_qt's table
    f29_qtab_init(qt);
    __syncthreads();
    const size_t i = gtid() / LANES;
    if (i >= nout) return;
    if (!LSP_BOUNDS(2 * i + 1 < 2 * nout)) return;
    const Fr row = inj[i];  // in flight behind the first permutation
    const Fr pair = compress_f29<D, LANES>(src[2 * i], src[2 * i + 1], rc, rf, rp, qt);
    const Fr d = compress_f29<D, LANES>(pair, row, rc, rf, rp, qt);
    if ((threadIdx.x & (LANES - 1)) == 0) dst[i] = d;
}
}  // namespace

// k_hash.hip's thresholds (lanes_for, state_grid) and their knobs
static size_t env_size(const char* name, size_t dflt) {
    const char* e = std::getenv(name);
    return e ? (size_t)std::strtoull(e, nullptr, 10) : dflt;
}
static int lanes_for(size_t n) {
    static const size_t coop_max = env_size("LSP_COOP_MAX", 16384), pair_max = env_size("LSP_PAIR_MAX", 32768);
    return n <= coop_max ? 4 : (n <= pair_max ? 2 : 1);
}
static void state_grid(size_t n, int lanes, unsigned& blocks, unsigned& bs) {
    static const unsigned coop_bs = (unsigned)env_size("LSP_COOP_BS", 0);
    bs = lanes == 4 ? (coop_bs ? coop_bs : (4 * n >= 65536 ? 256u : 64u)) : 256u;
    blocks = nblocks((size_t)lanes * n, bs);
}

#define LSP_INJECT_L(DEG, LANES)                                                                                   \
    hipLaunchKernelGGL((k_merkle_inject<DEG, LANES>), dim3(blocks), dim3(bs), 0, st, src, inj, dst, nout, rc, \
                       L.rounds_f, L.rounds_p)
#define LSP_INJECT_D(DEG)          \
    do {                           \
        if (lanes == 4)            \
            LSP_INJECT_L(DEG, 4);  \
        else if (lanes == 2)       \
            LSP_INJECT_L(DEG, 2);  \
        else                       \
            LSP_INJECT_L(DEG, 1);  \
    } while (0)

hipError_t launch_merkle_inject(const Fr* src, const Fr* inj, Fr* dst, size_t nout, const F29* rc, P2Layout L,
                                hipStream_t st) {
    if (!nout) return hipSuccess;
    const int lanes = lanes_for(nout);
    unsigned blocks, bs;
    state_grid(nout, lanes, blocks, bs);
    if (L.gen_lin) {
        if (L.sbox_degree == 17)
            LSP_INJECT_D(17u | P2_GEN);
        else
            LSP_INJECT_D(11u | P2_GEN);
    } else if (L.sbox_degree == 17)
        LSP_INJECT_D(17u);
    else
        LSP_INJECT_D(11u);
    return hipGetLastError();
}

}  // namespace lsp

LSP_BOUNDS_READER(k_merkle_inject)
