// FRI over inputs of unequal heights: the fold of a
// round with the roll-in fused -- where a reduced-opening vector `add` is as
// long as the folded vector, v'[i] = fold(v)[i] + add[i] (plain addition, the
// fork's p3-fri) -- and, in k_fold_add_hash, the next round's leaves over v'.
//
// A translation unit of its own, so that adding it left k_hash.hip's kernels
// as compiled before (profiles/pcs_codegen.txt).  k_fold_add_hash is
// k_fold_hash (k_hash.hip) with one nullable operand more; the launcher takes
// its lane form and grid from p2_launch.hpp, as k_hash.hip's do: a fused leaf
// batch takes the lane form a plain leaf batch of its size takes.
#include "k_common.hpp"
#include "kernels.hpp"
#include "p2_launch.hpp"
#include "poseidon2_f29.hpp"

namespace lsp {

namespace {
// launch_fri_fold's formula for output i of the fold `f` describes, plus add[i]
// (add nullable).  fr_add of two reduced values is reduced: what is stored is
// canonical, as everywhere in memory.
__device__ __forceinline__ Fr fold_add_at(const FoldSpec& f, const Fr* __restrict__ add, size_t i) {
    const Fr p = fr_mul(f.half_beta, pow2l(f.tab, f.L1, brev_bits(f.i0 + i, f.logm)));
    const Fr e = fr_add(fr_mul(fr_add(f.half, p), f.v[2 * i]), fr_mul(fr_sub(f.half, p), f.v[2 * i + 1]));
    return add ? fr_add(e, add[i]) : e;
}

// LANES: lanes per leaf -- 4 (a DPP quad), 2 (a pair) or 1, as in k_fold_hash.
// Every lane of a leaf computes both values (the sponge reads them from
// registers); the lead lane alone stores them.
template <uint32_t D, int LANES>
__global__ __launch_bounds__(256) void k_fold_add_hash(FoldSpec f, const Fr* __restrict__ add, size_t nleaves,
                                                       Fr* __restrict__ out, const F29* __restrict__ rc, uint32_t rf,
                                                       uint32_t rp) {
    __shared__ uint4 qt[3 * F29_QTAB_N];  // f29_reduce_qt's table
    f29_qtab_init(qt);
    __syncthreads();
    const size_t j = gtid() / LANES;
    if (j >= nleaves) return;
    if (!LSP_BOUNDS(2 * j + 1 < 2 * nleaves)) return;
    Fr e[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) e[k] = fold_add_at(f, add, 2 * j + k);
    if ((threadIdx.x & (LANES - 1)) == 0) {
        f.vout[2 * j] = e[0];
        f.vout[2 * j + 1] = e[1];
    }
    const Fr d = sponge_f29<D, LANES>([&](uint32_t k) { return e[k]; }, 2, rc, rf, rp, qt);
    if ((threadIdx.x & (LANES - 1)) == 0) out[j] = d;
}

// the last fold, which no leaf kernel follows
__global__ __launch_bounds__(256) void k_fri_fold_add(FoldSpec f, const Fr* __restrict__ add, size_t m) {
    const size_t i = gtid();
    if (i >= m) return;
    f.vout[i] = fold_add_at(f, add, i);
}
}  // namespace

hipError_t launch_fold_add_hash(const FoldSpec& f, const Fr* add, size_t nleaves, Fr* out, const F29* rc, P2Layout L,
                                hipStream_t st) {
    if (!nleaves) return hipSuccess;
    const int lanes = lanes_for(nleaves);
    unsigned blocks, bs;
    state_grid(nleaves, lanes, blocks, bs);
    p2_dispatch(L, lanes, [&](auto d, auto ln) {
        hipLaunchKernelGGL((k_fold_add_hash<decltype(d)::value, decltype(ln)::value>), dim3(blocks), dim3(bs), 0, st, f,
                           add, nleaves, out, rc, L.rounds_f, L.rounds_p);
    });
    return hipGetLastError();
}

hipError_t launch_fri_fold_add(const FoldSpec& f, const Fr* add, size_t m, hipStream_t st) {
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(k_fri_fold_add, dim3(nblocks(m, 256)), dim3(256), 0, st, f, add, m);
    return hipGetLastError();
}

}  // namespace lsp

LSP_BOUNDS_READER(k_fri_mixed)
