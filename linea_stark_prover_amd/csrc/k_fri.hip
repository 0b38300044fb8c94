// The FRI fold (TwoAdicFriGenericConfig::fold_matrix) on the device, once:
// fold_at holds the formula and the roll-in of a reduced-opening vector where
// the lengths meet (plain addition, the fork's
// p3-fri).  Two kernels call it: k_fold_hash, which also hashes the folded
// vector's pairs into the next round's leaves, and k_fri_fold, the fold no leaf
// kernel follows.
//
// A translation unit of its own: k_hash.hip's and k_open.hip's other kernels
// compile as they did before these two moved here (profiles/fri_codegen.txt).
// The launcher of k_fold_hash takes its lane form and grid from p2_launch.hpp,
// as k_hash.hip's do: a fused leaf batch takes the lane form a plain leaf batch
// of its size takes.
#include "k_common.hpp"
#include "kernels.hpp"
#include "p2_launch.hpp"
#include "poseidon2_f29.hpp"

namespace lsp {

namespace {
// output i of the fold `f` describes: (half + p) v[2i] + (half - p) v[2i+1],
// p = half_beta * tab^bitrev_logm(i0 + i), plus add[i] with ADD.  fr_add of two
// reduced values is reduced: what is stored is canonical, as everywhere in
// memory.  ADD is a template parameter the launchers set from f.add: tested at
// run time, the one more live pointer cost the fused kernel's narrow forms up
// to two waves per SIMD (profiles/fri_codegen.txt).
template <bool ADD>
__device__ __forceinline__ Fr fold_at(const FoldSpec& f, size_t i) {
    const Fr p = fr_mul(f.half_beta, pow2l(f.tab, f.L1, brev_bits(f.i0 + i, f.logm)));
    const Fr e = fr_add(fr_mul(fr_add(f.half, p), f.v[2 * i]), fr_mul(fr_sub(f.half, p), f.v[2 * i + 1]));
    if constexpr (ADD) {
        const Fr* __restrict__ add = f.add;
        return fr_add(e, add[i]);
    }
    return e;
}

// LANES: lanes per leaf -- 4 (a DPP quad), 2 (a pair) or 1, as in k_hash_rows1.
// Every lane of a leaf computes both values (the sponge reads them from
// registers); the lead lane alone stores them.
template <uint32_t D, int LANES, bool ADD>
__global__ __launch_bounds__(256) void k_fold_hash(FoldSpec f, size_t nleaves, Fr* __restrict__ out,
                                                   const F29* __restrict__ rc, uint32_t rf, uint32_t rp) {
    __shared__ uint4 qt[3 * F29_QTAB_N];  // f29_reduce_qt's table
    f29_qtab_init(qt);
    __syncthreads();
    const size_t j = gtid() / LANES;
    if (j >= nleaves) return;
    if (!LSP_BOUNDS(2 * j + 1 < 2 * nleaves)) return;
    Fr e[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) e[k] = fold_at<ADD>(f, 2 * j + k);
    if ((threadIdx.x & (LANES - 1)) == 0) {
        f.vout[2 * j] = e[0];
        f.vout[2 * j + 1] = e[1];
    }
    const Fr d = sponge_f29<D, LANES>([&](uint32_t k) { return e[k]; }, 2, rc, rf, rp, qt);
    if ((threadIdx.x & (LANES - 1)) == 0) out[j] = d;
}

template <bool ADD>
__global__ __launch_bounds__(256) void k_fri_fold(FoldSpec f, size_t m) {
    const size_t i = gtid();
    if (i >= m) return;
    f.vout[i] = fold_at<ADD>(f, i);
}
}  // namespace

hipError_t launch_fold_hash(const FoldSpec& f, size_t nleaves, Fr* out, const F29* rc, P2Layout L, hipStream_t st) {
    if (!nleaves) return hipSuccess;
    const int lanes = lanes_for(nleaves);
    unsigned blocks, bs;
    state_grid(nleaves, lanes, blocks, bs);
    p2_dispatch(L, lanes, [&](auto d, auto ln) {
        constexpr uint32_t D = decltype(d)::value;
        constexpr int LN = decltype(ln)::value;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(f.add ? k_fold_hash<D, LN, true> : k_fold_hash<D, LN, false>), dim3(blocks),
                           dim3(bs), 0, st, f, nleaves, out, rc, L.rounds_f, L.rounds_p);
    });
    return hipGetLastError();
}

hipError_t launch_fri_fold(const FoldSpec& f, size_t m, hipStream_t st) {
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(f.add ? k_fri_fold<true> : k_fri_fold<false>, dim3(nblocks(m, 256)), dim3(256), 0, st, f, m);
    return hipGetLastError();
}

}  // namespace lsp

LSP_BOUNDS_READER(k_fri)
