// The columns of a witness block, the only place that knows their order:
//
//   permutation (RawPermutationTrace::get_trace, trace/src/permutation.rs:81-90)
//       a[na], b[nb], b_inverse, check
//   lookup (RawLookupTrace::get_trace, trace/src/lookup.rs:162-214)
//       a[na], b[nt][nbc], a_filter, b_filter[nt], a_inverse, b_inverse[nt],
//       multiplicity[nt], sum
//
// A block starts with its raw input columns in the order a raw block holds
// them column-major (a | b | a_filter | b_filter): raw_*() are offsets in
// columns into such a block, raw_cols() its size.  describe() writes the
// block's LSP_AIR_PERMUTATION / LSP_AIR_LOOKUP config (include/lsp.h) with the
// ids shifted by col0 -- the words air_walk.hpp's air_decode reads.
//
// No HIP types here: the members are constexpr, so under hipcc the kernels of
// k_witness.hip call the same ones as the host generators and the C entry
// points (witness.cpp) and the CBOR reader (cbor.cpp), and
// tests/witness_layout_check.cpp builds with the host compiler alone.  Column
// ids are 32-bit: with 64-bit ids k_lookup_rows loses a wave of occupancy
// (profiles/witness_codegen.txt); sizes are size_t.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/lsp.h"

namespace lsp {

struct PermBlock {
    uint32_t na, nb;
    constexpr uint32_t a(uint32_t k) const { return k; }
    constexpr uint32_t b(uint32_t k) const { return na + k; }
    constexpr uint32_t b_inv() const { return b(nb); }
    constexpr uint32_t check() const { return b_inv() + 1; }

    constexpr size_t raw_a() const { return 0; }
    constexpr size_t raw_b() const { return na; }
    constexpr size_t raw_cols() const { return (size_t)na + nb; }
    // = check() + 1, in 64 bits: counts that would wrap a column id miss the
    // caller's trace width (witness_block) instead
    constexpr size_t width() const { return raw_cols() + 2; }

    // type, na, nb, then the ids of all columns, which the descriptor lists in
    // the block's own order; describe returns the end of its words
    constexpr size_t desc_len() const { return 3 + width(); }
    constexpr int32_t* describe(size_t col0, int32_t* out) const {
        *out++ = LSP_AIR_PERMUTATION;
        *out++ = (int32_t)na;
        *out++ = (int32_t)nb;
        for (size_t c = a(0); c < width(); ++c) *out++ = (int32_t)(col0 + c);
        return out;
    }
};

struct LookupBlock {
    uint32_t na, nt, nbc;
    constexpr uint32_t a(uint32_t k) const { return k; }
    constexpr uint32_t b(uint32_t t, uint32_t c) const { return na + t * nbc + c; }
    constexpr uint32_t a_filter() const { return b(nt, 0); }
    constexpr uint32_t b_filter(uint32_t t) const { return a_filter() + 1 + t; }
    constexpr uint32_t a_inv() const { return b_filter(nt); }
    constexpr uint32_t b_inv(uint32_t t) const { return a_inv() + 1 + t; }
    constexpr uint32_t mult(uint32_t t) const { return b_inv(nt) + t; }
    constexpr uint32_t sum() const { return mult(nt); }

    constexpr size_t raw_a() const { return 0; }
    constexpr size_t raw_b() const { return na; }
    constexpr size_t raw_a_filter() const { return raw_b() + (size_t)nt * nbc; }
    constexpr size_t raw_b_filter() const { return raw_a_filter() + 1; }
    constexpr size_t raw_cols() const { return raw_b_filter() + nt; }
    // = sum() + 1, in 64 bits (see PermBlock::width): the raw columns, 1 + nt
    // inverses, nt multiplicities, the sum
    constexpr size_t width() const { return raw_cols() + 2 * (size_t)nt + 2; }

    // type, na, a's ids, nt, nbc, then the ids of the other columns, again in the block's order
    constexpr size_t desc_len() const { return 4 + width(); }
    constexpr int32_t* describe(size_t col0, int32_t* out) const {
        *out++ = LSP_AIR_LOOKUP;
        *out++ = (int32_t)na;
        for (size_t c = a(0); c < b(0, 0); ++c) *out++ = (int32_t)(col0 + c);
        *out++ = (int32_t)nt;
        *out++ = (int32_t)nbc;
        for (size_t c = b(0, 0); c < width(); ++c) *out++ = (int32_t)(col0 + c);
        return out;
    }
};

}  // namespace lsp
