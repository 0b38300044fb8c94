// p3-uni-stark check_constraints on the device: LineaAIR::eval
// (air/src/lib.rs:47-167) on every pair of adjacent rows of the trace itself,
// which the reference's debug build runs inside p3_uni_stark::prove
// (bin/src/main.rs:80-86) and panics from with the first failing row.
//
// Thread i checks row i of the row-major h x w trace in natural order (no LDE,
// no bit reversal): local = row i, next = row (i + 1) mod h, with the 0/1
// selectors is_first_row = (i == 0), is_last_row = (i == h - 1), is_transition
// = (i != h - 1).  The AIR is the int32 descriptor of include/lsp.h, walked
// with wave-uniform control flow in the constraint order of k_quotient.hip's
// PUSH (the selectors are data, never branches), so every lane of a wave
// reaches every ballot.  A wave's 64 lanes read 64 adjacent rows and their
// successors: each row is read by two lanes of one wave (the wave's last
// lane shares its `next` with the following wave), few products per byte.
//
// Outputs, all through vector stores and vector atomics:
//   row_mask[i / 64] bit i % 64   row i violates a constraint: one ballot per
//                                 wave, stored by its first lane
//   count[j]                      rows violating constraint j: a ballot per
//                                 constraint, one atomicAdd of its popcount by
//                                 the wave's first lane, only when nonzero
//   first_row[j]                  the lowest such row: atomicMin of the wave's
//                                 lowest set lane, beside that atomicAdd
// A valid trace issues no atomic; a trace on which every row fails issues
// h / 64 per constraint.  Sums and minima do not depend on the order the waves
// run in.  k_check_rows re-evaluates a short list of rows and writes every
// constraint's canonical value (the detail records of the report).
#include "fr29.hpp"
#include "k_air_prog.hpp"
#include "k_common.hpp"
#include "kernels.hpp"

namespace lsp {

namespace {
// v == 0 (mod r), exactly.  Bound: every value check_walk hands out is either
// the result of Q29::sub (f29_reduce_qt: normalised limbs, value < 2 r) or a
// loaded cell (Q29::load -> f29_reduce: limbs 0..7 masked to 29 bits, value < 2 r
// for any word below 2^256).  A normalised limb vector is the unique one of
// its integer, and the only multiples of r in [0, 2 r) are 0 and r: the value
// is zero mod r iff its limbs are all zero or are r's own limbs.  (The factor
// 2^261 of the representation does not move zero.)  No product is tested
// unreduced, so the < 8.92 r range of f29_mul's output never reaches here.
__device__ __forceinline__ bool f29_is_zero_mod_r(const F29& v) {
    uint32_t z = 0, e = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        z |= v.l[i];
        e |= v.l[i] ^ p29(i);
    }
    return z == 0 || e == 0;
}

// LineaAIR::eval on one row pair: push(value, selector) per constraint in
// eval's order, value normalised and < 2 r, not multiplied by the selector
// (the built-in configs: air_walk over Q29, the selector tag turned into the
// row's 0/1).  i, in: the rows `loc` and `nxt` are (a program reads the preprocessed matrix
// at the same two).
// PROG: also run LSP_AIR_PROGRAM configs (k_air_prog.hpp; an instantiation of
// its own, as in k_quotient.hip).  A program takes the 0/1 selectors as data
// wherever it names them, so its asserts are pushed under `always`; an asserted
// operand may be a raw product (< 8.92 r), a selector or a constant, and goes
// through one reduction first (normalised, < 2 r: what the zero test needs).
template <bool PROG, class Push>
__device__ __forceinline__ void check_walk(const Q29& F, const CheckArgs& a, const Fr* __restrict__ loc,
                                           const Fr* __restrict__ nxt, uint64_t i, uint64_t in, bool first, bool last,
                                           Push&& push) {
    const bool trans = !last;
    const F29 ap = f29_from_fr(a.pub_alpha), dl = f29_from_fr(a.pub_delta);
    AirWords d{a.air, 0};
    const int32_t ncfg = d.word();
    for (int32_t c = 0; c < ncfg; ++c) {
        const int32_t type = d.word();
        if (!PROG || type != LSP_AIR_PROGRAM) {
            air_walk(F, type, d, loc, nxt, ap, dl, [&](const F29& v, auto sel, AirCons) {
                constexpr Sel s = decltype(sel)::value;
                push(v, s == Sel::Always || (s == Sel::First ? first : s == Sel::Trans ? trans : last));
            });
        } else if constexpr (PROG) {
            extern __shared__ uint32_t prog_regs[];
            const F29 zero = f29_zero(), one = F.one();
            const ProgEnv e{loc,
                            nxt,
                            a.w,
                            a.pub,
                            a.npub,
                            first ? one : zero,
                            last ? one : zero,
                            trans ? one : zero,
                            prog_regs,
                            a.prog_slots,
                            a.prep + i * a.wp,  // (rows i and in of the h x wp matrix)
                            a.prep + in * a.wp,
                            a.wp};
            d.p = air_prog_run(F, e, d.d, d.p, [&](const F29& v) { push(f29_reduce_qt(v, F.qt), true); });
        }
    }
}

template <bool PROG>
__global__ __launch_bounds__(256) void k_check(CheckArgs a) {
    __shared__ uint4 qt[3 * F29_QTAB_N];  // f29_reduce_qt's table
    f29_qtab_init(qt);
    __syncthreads();
    const Q29 F{qt, a.w};
    const uint64_t t = gtid();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t row0 = t - lane;  // the wave's first row
    if (row0 >= a.h) return;         // a whole wave past the last row
    // lanes past the last row of a partial wave walk row 0 and report nothing:
    // the ballots need every lane
    const bool live = t < a.h;
    const uint64_t i = live ? t : 0;
    const uint64_t in = i + 1 == a.h ? 0 : i + 1;
    const Fr* loc = a.trace + i * a.w;
    const Fr* nxt = a.trace + in * a.w;
    unsigned long long* count = reinterpret_cast<unsigned long long*>(a.count);
    unsigned long long* first_row = reinterpret_cast<unsigned long long*>(a.first_row);
    uint32_t j = 0;
    bool any = false;
    check_walk<PROG>(F, a, loc, nxt, i, in, i == 0, i + 1 == a.h, [&](const F29& v, bool sel) {
        const bool bad = live && sel && !f29_is_zero_mod_r(v);
        const unsigned long long m = __ballot(bad);
        any |= bad;
        if (m != 0 && lane == 0 && LSP_BOUNDS(j < a.ncons)) {
            atomicAdd(count + j, (unsigned long long)__popcll(m));
            atomicMin(first_row + j, (unsigned long long)(row0 + (uint64_t)(__ffsll((long long)m) - 1)));
        }
        ++j;
    });
    const unsigned long long m = __ballot(any);
    if (lane == 0 && LSP_BOUNDS(row0 / 64 < (a.h + 63) / 64)) a.row_mask[row0 / 64] = m;
}

template <bool PROG>
__global__ __launch_bounds__(64) void k_check_rows(CheckArgs a) {
    __shared__ uint4 qt[3 * F29_QTAB_N];
    f29_qtab_init(qt);
    __syncthreads();
    const Q29 F{qt, a.w};
    const uint64_t t = gtid();
    bool live = t < a.nrows;
    uint64_t i = live ? a.rows[t] : 0;
    if (!LSP_BOUNDS(i < a.h)) {
        live = false;
        i = 0;
    }
    const uint64_t in = i + 1 == a.h ? 0 : i + 1;
    uint32_t j = 0;
    check_walk<PROG>(F, a, a.trace + i * a.w, a.trace + in * a.w, i, in, i == 0, i + 1 == a.h,
                     [&](const F29& v, bool sel) {
        const Fr x = f29_to_fr_qt(v, qt);  // canonical, ark form
        if (live && LSP_BOUNDS(j < a.ncons)) a.vals[t * a.ncons + j] = sel ? x : fr_zero();
        ++j;
    });
}
}  // namespace

hipError_t launch_check(const CheckArgs& a, hipStream_t st) {
    if (!a.h || !a.row_mask || !a.count || !a.first_row) return hipErrorInvalidValue;
    if (a.wp && (!a.prep || !a.prog)) return hipErrorInvalidValue;
    if (a.prog) {
        if (!a.pub || a.npub < 2 || a.prog_slots > 16) return hipErrorInvalidValue;
        const uint32_t bs = air_prog_block(a.prog_slots);
        return launch_lds(k_check<true>, nblocks(a.h, bs), bs, air_prog_lds_bytes(a.prog_slots, bs), st, a);
    }
    hipLaunchKernelGGL(k_check<false>, dim3(nblocks(a.h, 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_check_rows(const CheckArgs& a, hipStream_t st) {
    if (!a.h || !a.nrows || !a.rows || !a.vals) return hipErrorInvalidValue;
    if (a.wp && (!a.prep || !a.prog)) return hipErrorInvalidValue;
    if (a.prog) {  // 64 threads: 16 slots are 36 KB
        if (!a.pub || a.npub < 2 || a.prog_slots > 16) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_check_rows<true>, dim3(nblocks(a.nrows, 64)), dim3(64),
                           air_prog_lds_bytes(a.prog_slots, 64), st, a);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_check_rows<false>, dim3(nblocks(a.nrows, 64)), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace lsp

LSP_BOUNDS_READER(k_check)
