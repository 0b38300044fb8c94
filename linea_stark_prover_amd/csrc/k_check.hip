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
// the 29-bit-limb arithmetic of k_quotient.hip's Q29, at the same bounds: add /
// sub inputs < 20 r give < 40 r with limbs < 1.5 2^30 (f29_reduce_qt takes
// < 64 r, limbs < 2.41 2^30) and leave normalised and < 2 r; f29_sub16 takes a
// subtrahend < 16 r; products (< 8.92 r for inputs < 20 r) stay as the
// multiplier leaves them
struct Q29 {
    const uint4* qt;
    __device__ __forceinline__ F29 add(const F29& a, const F29& b) const { return f29_reduce_qt(f29_lazy2(a, b), qt); }
    __device__ __forceinline__ F29 sub(const F29& a, const F29& b) const { return f29_reduce_qt(f29_sub16(a, b), qt); }
    __device__ __forceinline__ F29 mul(const F29& a, const F29& b) const { return f29_mul(a, b); }
};

// column k of a row (lsp_check_constraints checks the descriptor's ids against
// the width before any launch; the debug build checks them again here)
__device__ __forceinline__ F29 ld29(const Fr* __restrict__ row, int32_t k, uint32_t w) {
    return LSP_BOUNDS(k >= 0 && (uint32_t)k < w) ? f29_from_fr(row[k]) : f29_zero();
}

__device__ __forceinline__ F29 horner(const Q29& F, const Fr* __restrict__ row, const int32_t* __restrict__ ids,
                                      int32_t n, const F29& a, uint32_t w) {
    F29 acc = f29_zero();
    for (int32_t k = 0; k < n; ++k) acc = F.add(F.mul(acc, a), ld29(row, ids[k], w));
    return acc;
}

// v == 0 (mod r), exactly.  Bound: every value check_walk hands out is either
// the result of Q29::sub (f29_reduce_qt: normalised limbs, value < 2 r) or a
// loaded cell (ld29 -> f29_reduce: limbs 0..7 masked to 29 bits, value < 2 r
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
// eval's order, value normalised and < 2 r, not multiplied by the selector.
// i, in: the rows `loc` and `nxt` are (a program reads the preprocessed matrix
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
    const bool trans = !last, always = true;
    const F29 one = f29_from_fr(fr_one());
    const F29 ap = f29_from_fr(a.pub_alpha), dl = f29_from_fr(a.pub_delta);
    const int32_t* d = a.air;
    int32_t p = 0;
    const int32_t ncfg = d[p++];
    for (int32_t c = 0; c < ncfg; ++c) {
        const int32_t type = d[p++];
        if (type == 1) {  // AirPermutationConfig: air/src/lib.rs:116-167
            const int32_t na = d[p++], nb = d[p++];
            const int32_t* aid = d + p;
            p += na;
            const int32_t* bid = d + p;
            p += nb;
            const int32_t binv = d[p++], chk = d[p++];
            const F29 a_l = F.add(horner(F, loc, aid, na, ap, a.w), dl);
            const F29 b_l = F.add(horner(F, loc, bid, nb, ap, a.w), dl);
            const F29 lbinv = ld29(loc, binv, a.w), lchk = ld29(loc, chk, a.w);
            push(F.sub(F.mul(b_l, lbinv), one), always);
            push(F.sub(lchk, F.mul(a_l, lbinv)), first);
            const F29 a_n = F.add(horner(F, nxt, aid, na, ap, a.w), dl);
            push(F.sub(ld29(nxt, chk, a.w), F.mul(F.mul(lchk, a_n), ld29(nxt, binv, a.w))), trans);
            push(F.sub(lchk, one), last);
        } else if (!PROG || type == 2) {  // AirLookupConfig: air/src/lib.rs:57-114
            const int32_t na = d[p++];
            const int32_t* aid = d + p;
            p += na;
            const int32_t nt = d[p++], nbc = d[p++];
            const int32_t* bid = d + p;
            p += nt * nbc;
            const int32_t afil = d[p++];
            const int32_t* bfil = d + p;
            p += nt;
            const int32_t ainv = d[p++];
            const int32_t* binv = d + p;
            p += nt;
            const int32_t* occ = d + p;
            p += nt;
            const int32_t chk = d[p++];
            const F29 a_l = F.add(horner(F, loc, aid, na, ap, a.w), dl);
            const F29 lainv = ld29(loc, ainv, a.w);
            push(F.sub(F.mul(a_l, lainv), one), always);
            F29 lc = F.mul(ld29(loc, afil, a.w), lainv);
            F29 nc = F.mul(ld29(nxt, afil, a.w), ld29(nxt, ainv, a.w));
            for (int32_t t = 0; t < nt; ++t) {
                const F29 b_l = F.add(horner(F, loc, bid + t * nbc, nbc, ap, a.w), dl);
                const F29 lbinv = ld29(loc, binv[t], a.w);
                push(F.sub(F.mul(b_l, lbinv), one), always);
                lc = F.sub(lc, F.mul(F.mul(ld29(loc, bfil[t], a.w), ld29(loc, occ[t], a.w)), lbinv));
                nc = F.sub(nc, F.mul(F.mul(ld29(nxt, bfil[t], a.w), ld29(nxt, occ[t], a.w)), ld29(nxt, binv[t], a.w)));
            }
            const F29 lchk = ld29(loc, chk, a.w);
            push(F.sub(lchk, lc), first);
            push(F.sub(F.sub(ld29(nxt, chk, a.w), lchk), nc), trans);
            push(lchk, last);
        } else if constexpr (PROG) {
            extern __shared__ uint32_t prog_regs[];
            const F29 zero = f29_zero();
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
            p = air_prog_run(F, e, d, p, [&](const F29& v) { push(f29_reduce_qt(v, F.qt), always); });
        }
    }
}

template <bool PROG>
__global__ __launch_bounds__(256) void k_check(CheckArgs a) {
    __shared__ uint4 qt[3 * F29_QTAB_N];  // f29_reduce_qt's table
    f29_qtab_init(qt);
    __syncthreads();
    const Q29 F{qt};
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
    const Q29 F{qt};
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
        const size_t lds = air_prog_lds_bytes(a.prog_slots, bs);
        if (lds > 48 * 1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_check<true>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_check<true>, dim3(nblocks(a.h, bs)), dim3(bs), lds, st, a);
        return hipGetLastError();
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
