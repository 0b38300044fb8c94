// The interpreter of LSP_AIR_PROGRAM configs (include/lsp.h), shared by the
// program-capable instantiations of k_quotient.hip and k_check.hip: a
// straight-line program of ADD / SUB / MUL over field registers ("slots") whose
// ASSERT_ZERO ops hand out the constraint values in order.
//
// Device form of a config (Air::parse writes it, Air::dev): the descriptor's
// words with every constant replaced by the nine 29-bit limbs of its 2^261
// form, canonical -- so a constant operand is nine scalar loads and no
// conversion:
//   3, width, nslots, nconst, nops, nassert, const[nconst][9], op[nops][4]
// An LSP_AIR_PROGRAM_PREP config takes the same form (type word 3, prep_width
// dropped): its PREP_LOCAL / PREP_NEXT operands read the preprocessed matrix
// of the launch, whose width the host has checked against every prep_width.
//
// Register file: LDS, not an indexed local array (the compiler sends a
// runtime-indexed array to scratch).  Limb-planar: slot s, limb l of thread t
// at regs[(s * 9 + l) * blockDim.x + t], so a wave's 64 lanes read 64
// adjacent words (no bank conflict), 36 bytes x blockDim.x per slot, sized by
// the launch from the largest nslots of the descriptor (dynamic shared
// memory).  A thread touches only its own column: no barrier.
//
// Control flow is wave-uniform: opcode, operand kinds and payloads come from
// the descriptor, which every lane reads at the same index, so every lane
// executes every op (k_check's ballots rely on it) and the descriptor reads
// are scalar loads.
//
// Bounds of the arithmetic (Q29 below, fr29.hpp).  An operand is
//   a loaded cell or public value   f29_from_fr: normalised, < 2 r (a cell of
//                                   the trace or of the preprocessed matrix)
//   a constant                      canonical: normalised, < r
//   a selector                      the quotient's are products (< 8.92 r) or
//                                   x - w^-1 (< 2 r); the check's are 0 or 1
//   a slot                          the result of an earlier op: add / sub
//                                   leave normalised and < 2 r, mul normalised
//                                   and < 8.92 r
// so every operand is normalised and < 8.92 r.  add takes two of them (sum
// < 17.84 r, limbs < 2^30; f29_reduce_qt takes < 64 r, limbs < 2.41 2^30),
// sub a subtrahend < 16 r (a + 16 r - b < 24.92 r, limbs < 1.5 2^30), mul
// inputs < 20 r.  The op set is closed: whatever a program computes, no op
// sees a value outside what it accepts (tests/test_air_program.py models it).
#pragma once
#include "air_walk.hpp"
#include "fr29.hpp"
#include "k_common.hpp"

namespace lsp {

// The algebra the kernels walk an AIR over (air_walk.hpp), on the 29-bit-limb
// product (fr29.hpp; ~2x the 8 x 32-bit product's rate): every trace value and
// constant enters in the 29-bit form (x 2^261: a repack and a cheap reduction
// from the ark form), sums and differences leave through the LDS-table
// reduction (< 2 r, normalised), products stay as the multiplier leaves them
// (normalised, < 8.92 r for inputs < 20 r).  Bounds: add / sub inputs < 20 r
// give < 40 r with limbs < 1.5 2^30 (f29_reduce_qt takes < 64 r, limbs
// < 2.41 2^30); f29_sub16 takes a subtrahend < 16 r.
struct Q29 {
    using V = F29;
    const uint4* qt;  // f29_reduce_qt's table
    uint32_t w;       // row width
    __device__ __forceinline__ F29 zero() const { return f29_zero(); }
    __device__ __forceinline__ F29 one() const { return f29_from_fr(fr_one()); }
    __device__ __forceinline__ F29 add(const F29& a, const F29& b) const { return f29_reduce_qt(f29_lazy2(a, b), qt); }
    __device__ __forceinline__ F29 sub(const F29& a, const F29& b) const { return f29_reduce_qt(f29_sub16(a, b), qt); }
    __device__ __forceinline__ F29 mul(const F29& a, const F29& b) const { return f29_mul(a, b); }
    // column k of a row (the host checks the descriptor's ids against the
    // width before any launch, Air::require_fits; the debug build checks them
    // again here)
    __device__ __forceinline__ F29 load(const Fr* __restrict__ row, int32_t k) const {
        return LSP_BOUNDS(k >= 0 && (uint32_t)k < w) ? f29_from_fr(row[k]) : f29_zero();
    }
};

// what one thread evaluates a program on
struct ProgEnv {
    const Fr* loc;
    const Fr* nxt;
    uint32_t w;          // row width (the host has checked every column against it)
    const Fr* pub;       // device table of the public values
    uint32_t npub;
    F29 first, last, trans;  // the selector operands
    uint32_t* regs;      // the block's register file
    uint32_t lds_slots;  // slots it was sized for
    // the same two rows of the preprocessed matrix (wp = 0: none; the host
    // refuses an AIR that reads one where the call has none)
    const Fr* ploc;
    const Fr* pnxt;
    uint32_t wp;
};

__device__ __forceinline__ F29 prog_slot_ld(const ProgEnv& e, uint32_t s) {
    F29 v = f29_zero();
    if (!LSP_BOUNDS(s < e.lds_slots)) return v;
    const uint32_t* r = e.regs + (size_t)s * 9 * blockDim.x + threadIdx.x;
#pragma unroll
    for (int l = 0; l < 9; ++l) v.l[l] = r[(size_t)l * blockDim.x];
    return v;
}

__device__ __forceinline__ void prog_slot_st(const ProgEnv& e, uint32_t s, const F29& v) {
    if (!LSP_BOUNDS(s < e.lds_slots)) return;
    uint32_t* r = e.regs + (size_t)s * 9 * blockDim.x + threadIdx.x;
#pragma unroll
    for (int l = 0; l < 9; ++l) r[(size_t)l * blockDim.x] = v.l[l];
}

__device__ __forceinline__ F29 prog_operand(const ProgEnv& e, const int32_t* __restrict__ cst, uint32_t nconst,
                                            int32_t x) {
    const uint32_t kind = (uint32_t)x >> 24, v = (uint32_t)x & 0xffffffu;
    switch (kind) {
        case AIR_OPND_SLOT: return prog_slot_ld(e, v);
        case AIR_OPND_LOCAL: return LSP_BOUNDS(v < e.w) ? f29_from_fr(e.loc[v]) : f29_zero();
        case AIR_OPND_NEXT: return LSP_BOUNDS(v < e.w) ? f29_from_fr(e.nxt[v]) : f29_zero();
        case AIR_OPND_PUBLIC: return LSP_BOUNDS(v < e.npub) ? f29_from_fr(e.pub[v]) : f29_zero();
        case AIR_OPND_CONST: {
            F29 c = f29_zero();
            if (LSP_BOUNDS(v < nconst)) {
#pragma unroll
                for (int l = 0; l < 9; ++l) c.l[l] = (uint32_t)cst[(size_t)v * 9 + l];
            }
            return c;
        }
        case AIR_OPND_FIRST: return e.first;
        case AIR_OPND_LAST: return e.last;
        case AIR_OPND_PREP_LOCAL: return LSP_BOUNDS(v < e.wp) ? f29_from_fr(e.ploc[v]) : f29_zero();
        case AIR_OPND_PREP_NEXT: return LSP_BOUNDS(v < e.wp) ? f29_from_fr(e.pnxt[v]) : f29_zero();
        default: return e.trans;  // AIR_OPND_TRANS
    }
}

// Run the program config whose words follow its type word at d[p]; returns the
// index past the config.  on_assert(v) gets each ASSERT_ZERO's value as its
// operand stands (normalised, < 8.92 r), in order.
template <class Q, class Assert>
__device__ __forceinline__ int32_t air_prog_run(const Q& F, const ProgEnv& e, const int32_t* __restrict__ d, int32_t p,
                                                Assert&& on_assert) {
    const uint32_t nconst = (uint32_t)d[p + 2], nops = (uint32_t)d[p + 3];
    const int32_t* cst = d + p + 5;
    const int32_t* op = cst + (size_t)nconst * 9;
    for (uint32_t i = 0; i < nops; ++i, op += 4) {
        const int32_t code = op[0];
        const F29 x = prog_operand(e, cst, nconst, op[2]);
        if (code == AIR_OP_ASSERT_ZERO) {
            on_assert(x);
            continue;
        }
        const F29 y = prog_operand(e, cst, nconst, op[3]);
        prog_slot_st(e, (uint32_t)op[1],
                     code == AIR_OP_MUL ? F.mul(x, y) : code == AIR_OP_ADD ? F.add(x, y) : F.sub(x, y));
    }
    return p + 5 + (int32_t)(nconst * 9 + nops * 4);
}

// bytes of dynamic shared memory for a register file of `slots` slots
inline size_t air_prog_lds_bytes(uint32_t slots, uint32_t block) { return (size_t)slots * 9 * block * sizeof(uint32_t); }
// Block size of a program-capable launch.  Up to 8 slots: 256 threads (at 8
// slots 73.7 KB of slots + the 3 KB reduction table per block, two blocks =
// 8 waves per CU, 2 per SIMD, inside the CU's 160 KB).  9 to 16 slots take 324
// to 576 bytes per thread, so at most 7 down to 4 waves fit a CU whatever the
// block size: 128 threads keep the granularity fine (16 slots: two blocks of
// 73.7 KB, one wave per SIMD).
inline uint32_t air_prog_block(uint32_t slots) { return slots <= 8 ? 256u : 128u; }

}  // namespace lsp
