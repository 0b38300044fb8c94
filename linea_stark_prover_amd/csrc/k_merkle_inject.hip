// The injecting level of a mixed-height Merkle tree (p3-merkle-tree's
// compress_and_inject): where a class of shorter
// matrices has as many rows as the level has nodes,
//   dst[i] = compress(compress(src[2i], src[2i+1]), inj[i]),
// inj[i] = the sponge digest of row i of the class (launch_hash_rows).
//
// A translation unit of its own, so that adding it left k_hash.hip's kernels
// as compiled before (profiles/mixed_mmcs_codegen.txt).  The launcher takes its
// lane form and grid from p2_launch.hpp, as k_hash.hip's do: an injecting level
// takes the lane form a plain level of its width takes.
#include "k_common.hpp"
#include "kernels.hpp"
#include "p2_launch.hpp"
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

hipError_t launch_merkle_inject(const Fr* src, const Fr* inj, Fr* dst, size_t nout, const F29* rc, P2Layout L,
                                hipStream_t st) {
    if (!nout) return hipSuccess;
    const int lanes = lanes_for(nout);
    unsigned blocks, bs;
    state_grid(nout, lanes, blocks, bs);
    p2_dispatch(L, lanes, [&](auto d, auto ln) {
        hipLaunchKernelGGL((k_merkle_inject<decltype(d)::value, decltype(ln)::value>), dim3(blocks), dim3(bs), 0, st,
                           src, inj, dst, nout, rc, L.rounds_f, L.rounds_p);
    });
    return hipGetLastError();
}

}  // namespace lsp

LSP_BOUNDS_READER(k_merkle_inject)
