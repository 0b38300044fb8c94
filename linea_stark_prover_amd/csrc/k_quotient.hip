// Quotient evaluation over the LDE domain: p3-uni-stark quotient_values with
// ProverConstraintFolder, running LineaAIR::eval (air/src/lib.rs:47-167) for
// every point of the quotient coset GEN * H_Q.
//
// The AIR is the int32 AirConfig descriptor of include/lsp.h, interpreted
// with wave-uniform control flow (every lane walks the same configs); the
// folder's accumulation acc = acc*alpha + C_j (Horner, U10) runs in the
// constraint order of eval.  Row `local` is LDE row bitrev_Q(i) and `next`
// is bitrev_Q((i + 2^log_q) mod Q) (get_evaluations_on_domain +
// vertically_packed_row_pair).
//
// The built-in configs are air_walk (air_walk.hpp) over Q29 (k_air_prog.hpp),
// at the bounds given there: a constraint under a selector is pushed as
// selector * value, both factors < 20 r.  The quotient value leaves canonical
// in the ark form.
#include <cstdlib>

#include "fr29.hpp"
#include "k_air_prog.hpp"
#include "k_common.hpp"
#include "kernels.hpp"

namespace lsp {

namespace {
__global__ __launch_bounds__(256) void k_selector_denoms(const Fr* __restrict__ tabQ, uint32_t L1, Fr gen,
                                                         Fr wh_inv, size_t n, uint64_t i0, uint32_t log_step,
                                                         Fr* __restrict__ den) {
    const size_t m = gtid();
    if (m >= n) return;
    const uint64_t i = i0 + ((uint64_t)m << log_step);
    const Fr x = fr_mul(gen, pow2l(tabQ, L1, i));
    den[m] = fr_mul(fr_sub(x, fr_one()), fr_sub(x, wh_inv));
}

// one constraint value of thread t, limb-planar (QuotientArgs::cons)
__device__ __forceinline__ void st_cons(const QuotientArgs& a, uint32_t j, size_t t, size_t n, const F29& v) {
    if (!LSP_BOUNDS(j < a.ncons)) return;
    uint32_t* c = a.cons + (size_t)j * 9 * n + t;
#pragma unroll
    for (int l = 0; l < 9; ++l) c[(size_t)l * n] = v.l[l];
}

// EARLY: write the constraint values (QuotientArgs::cons) instead of folding them.
// PROG: also run LSP_AIR_PROGRAM configs (k_air_prog.hpp) -- an instantiation
// of its own, launched only for a descriptor that holds one, so that the walker
// of the built-in configs keeps its code, registers and LDS.
template <bool EARLY, bool PROG>
__global__ __launch_bounds__(256) void k_quotient(QuotientArgs a) {
    __shared__ uint4 qt[3 * F29_QTAB_N];  // f29_reduce_qt's table
    f29_qtab_init(qt);
    __syncthreads();
    const Q29 F{qt, a.w};
    const size_t t = gtid();
    const size_t Q = 1ull << a.logQ;
    const size_t npts = a.n ? a.n : Q;
    if (t >= npts) return;  // n = Q >> log_step points
    // Row order: thread t evaluates point m = bitrev(t), whose row bitrev_Q(i)
    // is row0 + t, so a wave reads 64 adjacent LDE rows (and their
    // successors).  In point order it read rows Q/64 apart: with the C3
    // trace's 5.9 KB rows their lines left the L2 before the lane came back
    // for the next columns (2^20 x 184: 63.5 -> 36.7 ms), and with narrow
    // rows past the caches' size every row is a DRAM page miss (round 3:
    // 2^22 x 8 5.7 -> 3.9 ms).  Point order (coalesced inv_den reads and out
    // writes) remains for A/B runs (row_order = 0).
    const size_t m = a.row_order ? brev_bits(t, a.logQ - a.log_step) : t;
    const uint64_t i = a.i0 + ((uint64_t)m << a.log_step);
    const uint32_t qmask = (1u << a.log_q) - 1;
    const Fr x = fr_mul(a.gen, pow2l(a.tabQ, a.L1, i));
    const Fr xm1 = fr_sub(x, fr_one());
    const Fr xml = fr_sub(x, a.wh_inv);
    const F29 zh = f29_from_fr(a.zh[i & qmask]), inv_den = f29_from_fr(a.inv_den[m]);
    const F29 xml29 = f29_from_fr(xml);
    const F29 first = F.mul(zh, F.mul(xml29, inv_den));              // Z_H / (x - 1)
    const F29 last = F.mul(zh, F.mul(f29_from_fr(xm1), inv_den));  // Z_H / (x - w^-1)
    const F29 trans = xml29;                                         // x - w^-1
    const uint64_t lrow = brev_bits(i, a.logQ) - a.row0;
    const uint64_t nrow = brev_bits((i + (1ull << a.log_q)) & (Q - 1), a.logQ) - (a.lde_next ? a.row0_next : a.row0);
    // the rows this rank holds (lde_rows = 0: not given, unchecked)
    if (!LSP_BOUNDS(a.lde_rows == 0 || (lrow < a.lde_rows && nrow < (a.lde_next ? a.lde_next_rows : a.lde_rows))))
        return;
    const Fr* loc = a.lde + lrow * a.w;
    const Fr* nxt = (a.lde_next ? a.lde_next : a.lde) + nrow * a.w;
    const F29 ap = f29_from_fr(a.pub_alpha), dl = f29_from_fr(a.pub_delta), al = f29_from_fr(a.alpha);
    F29 acc = f29_zero();
    uint32_t ncw = 0;  // constraints written (EARLY)
#define PUSH(X)                                     \
    do {                                            \
        if constexpr (EARLY)                        \
            st_cons(a, ncw++, t, npts, (X));        \
        else                                        \
            acc = F.add(F.mul(acc, al), (X));       \
    } while (0)
    AirWords d{a.air, 0};
    const int32_t ncfg = d.word();
    for (int32_t c = 0; c < ncfg; ++c) {
        const int32_t type = d.word();
        if (!PROG || type != LSP_AIR_PROGRAM) {
            air_walk(F, type, d, loc, nxt, ap, dl, [&](const F29& v, auto sel, AirCons) {
                constexpr Sel s = decltype(sel)::value;
                if constexpr (s == Sel::Always)
                    PUSH(v);
                else
                    PUSH(F.mul(s == Sel::First ? first : s == Sel::Trans ? trans : last, v));
            });
        } else if constexpr (PROG) {  // the selectors are operands, an assert's value is pushed as it stands
            extern __shared__ uint32_t prog_regs[];
            // the preprocessed matrix at the rows of `loc` and `nxt`
            const ProgEnv e{loc,        nxt,          a.w,
                            a.pub,      a.npub,       first,
                            last,       trans,        prog_regs,
                            a.prog_slots, a.prep + lrow * a.wp, a.prep + nrow * a.wp,
                            a.wp};
            d.p = air_prog_run(F, e, d.d, d.p, [&](const F29& v) { PUSH(v); });
        }
    }
#undef PUSH
    if constexpr (!EARLY) a.out[m] = f29_to_fr_qt(F.mul(acc, f29_from_fr(a.inv_zh[i & qmask])), qt);
}

// the fold of the values k_quotient<true> wrote: thread t reads its own
// (coalesced) and writes point m as k_quotient<false> would
__global__ __launch_bounds__(256) void k_quotient_fold(QuotientArgs a) {
    __shared__ uint4 qt[3 * F29_QTAB_N];
    f29_qtab_init(qt);
    __syncthreads();
    const Q29 F{qt, 0};  // (loads no row)
    const size_t t = gtid();
    const size_t npts = a.n ? a.n : (1ull << a.logQ);
    if (t >= npts) return;
    const size_t m = a.row_order ? brev_bits(t, a.logQ - a.log_step) : t;
    const uint64_t i = a.i0 + ((uint64_t)m << a.log_step);
    const uint32_t qmask = (1u << a.log_q) - 1;
    const F29 al = f29_from_fr(a.alpha);
    F29 acc = f29_zero();
    for (uint32_t j = 0; j < a.ncons; ++j) {
        const uint32_t* c = a.cons + (size_t)j * 9 * npts + t;
        F29 v;
#pragma unroll
        for (int l = 0; l < 9; ++l) v.l[l] = c[(size_t)l * npts];
        acc = F.add(F.mul(acc, al), v);
    }
    a.out[m] = f29_to_fr_qt(F.mul(acc, f29_from_fr(a.inv_zh[i & qmask])), qt);
}
}  // namespace

hipError_t launch_selector_denoms(const Fr* tabQ, uint32_t L1, Fr gen, Fr wh_inv, size_t n, Fr* den,
                                  hipStream_t st, uint64_t i0, uint32_t log_step) {
    hipLaunchKernelGGL(k_selector_denoms, dim3(nblocks(n, 256)), dim3(256), 0, st, tabQ, L1, gen, wh_inv, n, i0,
                       log_step, den);
    return hipGetLastError();
}

// Thread order: LDE row order (LSP_QUOTIENT_ORDER=point: point order; read per
// call).  Row order measured faster at every size (profiles/r03x_quotient_order.txt:
// 2^19 x 8 0.475 -> 0.45 ms, 2^22 x 8 5.7 -> 3.9 ms, rank 0 of 2^26 over 8 ranks
// 60 -> 26 ms): in point order a wave's 64 rows are Q/64 apart, and past the
// caches' size every row is a DRAM page miss.
static QuotientArgs with_order(const QuotientArgs& a) {
    QuotientArgs b = a;
    b.row_order = 1;
    if (const char* e = std::getenv("LSP_QUOTIENT_ORDER")) {
        if (e[0] == 'r') b.row_order = 1;
        if (e[0] == 'p') b.row_order = 0;
    }
    return b;
}

// The program-capable walker: its register file is dynamic shared memory sized
// by the descriptor's largest nslots (k_air_prog.hpp; above 48 KB from 6 slots
// up at 256 threads, launch_lds).
template <bool EARLY>
static hipError_t launch_quotient_prog_t(const QuotientArgs& b, size_t n, hipStream_t st) {
    if (!b.pub || b.npub < 2 || b.prog_slots > 16) return hipErrorInvalidValue;
    // a preprocessed matrix is the whole LDE, indexed like `lde` from row 0
    if (b.wp && (!b.prep || b.row0 || b.lde_next)) return hipErrorInvalidValue;
    const uint32_t bs = air_prog_block(b.prog_slots);
    return launch_lds(k_quotient<EARLY, true>, nblocks(n, bs), bs, air_prog_lds_bytes(b.prog_slots, bs), st, b);
}
static hipError_t launch_quotient_prog(const QuotientArgs& b, size_t n, hipStream_t st) {
    return b.cons ? launch_quotient_prog_t<true>(b, n, st) : launch_quotient_prog_t<false>(b, n, st);
}

hipError_t launch_quotient(const QuotientArgs& a, hipStream_t st) {
    const size_t n = a.n ? a.n : (1ull << a.logQ);
    const QuotientArgs b = with_order(a);
    if (a.prog) return launch_quotient_prog(b, n, st);
    if (a.cons)
        hipLaunchKernelGGL((k_quotient<true, false>), dim3(nblocks(n, 256)), dim3(256), 0, st, b);
    else
        hipLaunchKernelGGL((k_quotient<false, false>), dim3(nblocks(n, 256)), dim3(256), 0, st, b);
    return hipGetLastError();
}

hipError_t launch_quotient_fold(const QuotientArgs& a, hipStream_t st) {
    if (!a.cons) return hipErrorInvalidValue;
    const size_t n = a.n ? a.n : (1ull << a.logQ);
    hipLaunchKernelGGL(k_quotient_fold, dim3(nblocks(n, 256)), dim3(256), 0, st, with_order(a));
    return hipGetLastError();
}

}  // namespace lsp

LSP_BOUNDS_READER(k_quotient)
