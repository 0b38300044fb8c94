// LineaAIR::eval (air/src/lib.rs:47-167) for the two built-in configs of
// include/lsp.h, written once: the quotient kernel, the constraint checker's
// kernels, the verifier, the host checker and the degree / count / kind
// queries are all this walker over an algebra of their own.
//
// An algebra A supplies its value type A::V and
//   zero(), one()          the constants
//   add, sub, mul          on V
//   load(row, col)         the cell of a row (what a row is, is A's business)
// air_walk calls push(value, selector, what) once per constraint, in eval's
// order.  The value is not multiplied by its selector: `selector` is a
// compile-time tag (SelTag<Sel::...>), so a consumer picks what to do with it
// by `if constexpr` and gains no runtime branch; `what` names the constraint
// (LSP_CONSTRAINT_*, and the table of a lookup's b_inverse).
#pragma once
#include <stdint.h>

#include <type_traits>

#include "../../include/lsp.h"

namespace lsp {

// LSP_AIR_PROGRAM operands and opcodes (include/lsp.h)
enum : uint32_t {
    AIR_OPND_SLOT = 0, AIR_OPND_LOCAL = 1, AIR_OPND_NEXT = 2, AIR_OPND_PUBLIC = 3, AIR_OPND_CONST = 4,
    AIR_OPND_FIRST = 5, AIR_OPND_LAST = 6, AIR_OPND_TRANS = 7,
    // LSP_AIR_PROGRAM_PREP only: a cell of the preprocessed matrix
    AIR_OPND_PREP_LOCAL = 8, AIR_OPND_PREP_NEXT = 9
};
enum : int32_t { AIR_OP_ADD = 1, AIR_OP_SUB = 2, AIR_OP_MUL = 3, AIR_OP_ASSERT_ZERO = 4 };
constexpr uint32_t AIR_PROG_MAX_SLOTS = 16;

// the selector a constraint stands under (when_first_row, when_transition, when_last_row)
enum class Sel { Always, First, Trans, Last };
template <Sel S>
using SelTag = std::integral_constant<Sel, S>;

// what a pushed constraint is: LSP_CONSTRAINT_*, and the lookup table of a b_inverse (else -1)
struct AirCons {
    int32_t kind, table;
};

// One built-in config, decoded: column ids and pointers into the descriptor.
//   permutation   a[na], b[nbc], b_inv[0] (its one inverse column), check
//   lookup        a[na], b[ntab][nbc], a_filter, b_filter[ntab], a_inv,
//                 b_inv[ntab], occ[ntab], check
struct AirView {
    int32_t na, ntab, nbc;
    const int32_t *a, *b, *b_filter, *b_inv, *occ;
    int32_t a_filter, a_inv, check;
};

// a descriptor Air::parse has accepted, read as it stands
struct AirWords {
    const int32_t* d;
    int32_t p;
    __host__ __device__ __forceinline__ int32_t word() { return d[p++]; }
    __host__ __device__ __forceinline__ const int32_t* words(int64_t n) {
        const int32_t* r = d + p;
        p += (int32_t)n;
        return r;
    }
};

// The words of one built-in config after its type word (LSP_AIR_PERMUTATION,
// else LSP_AIR_LOOKUP), the only place that knows their layout.  R: word()
// gives the next word, words(n) a pointer to the next n (Air::parse's reader
// checks both against the descriptor's end).
template <class R>
__host__ __device__ __forceinline__ AirView air_decode(int32_t type, R& r) {
    AirView g{};
    g.na = r.word();
    if (type == LSP_AIR_PERMUTATION) {
        g.ntab = 1;
        g.nbc = r.word();
        g.a = r.words(g.na);
        g.b = r.words(g.nbc);
        g.b_inv = r.words(1);
    } else {
        g.a = r.words(g.na);
        g.ntab = r.word();
        g.nbc = r.word();
        g.b = r.words((int64_t)g.ntab * g.nbc);
        g.a_filter = r.word();
        g.b_filter = r.words(g.ntab);
        g.a_inv = r.word();
        g.b_inv = r.words(g.ntab);
        g.occ = r.words(g.ntab);
    }
    g.check = r.word();
    return g;
}

// sum of row[ids[k]] alpha^(n-1-k) + delta, the accumulator starting from the constant zero
template <class A, class Row>
__host__ __device__ __forceinline__ typename A::V air_combo(const A& F, Row row, const int32_t* __restrict__ ids,
                                                            int32_t n, const typename A::V& alpha,
                                                            const typename A::V& delta) {
    typename A::V acc = F.zero();
    for (int32_t k = 0; k < n; ++k) acc = F.add(F.mul(acc, alpha), F.load(row, ids[k]));
    return F.add(acc, delta);
}

// The built-in config of type `type` whose words `r` stands at (left past them).
// Each arm decodes its own config: one decode ahead of the branch cost k_check
// a fifth of its rate on the wide AIR (profiles/air_walk_ab.txt).
template <class A, class R, class Row, class Push>
__host__ __device__ __forceinline__ void air_walk(const A& F, int32_t type, R& r, Row loc, Row nxt,
                                                  const typename A::V& alpha, const typename A::V& delta,
                                                  Push&& push) {
    using V = typename A::V;
    constexpr SelTag<Sel::Always> always{};
    constexpr SelTag<Sel::First> first{};
    constexpr SelTag<Sel::Trans> trans{};
    constexpr SelTag<Sel::Last> last{};
    const V one = F.one();
    if (type == LSP_AIR_PERMUTATION) {  // AirPermutationConfig: air/src/lib.rs:116-167
        const AirView g = air_decode(LSP_AIR_PERMUTATION, r);
        const V a_l = air_combo(F, loc, g.a, g.na, alpha, delta);
        const V b_l = air_combo(F, loc, g.b, g.nbc, alpha, delta);
        const V lbinv = F.load(loc, g.b_inv[0]), lchk = F.load(loc, g.check);
        push(F.sub(F.mul(b_l, lbinv), one), always, AirCons{LSP_CONSTRAINT_B_INVERSE, -1});
        push(F.sub(lchk, F.mul(a_l, lbinv)), first, AirCons{LSP_CONSTRAINT_FIRST_ROW, -1});
        const V a_n = air_combo(F, nxt, g.a, g.na, alpha, delta);
        push(F.sub(F.load(nxt, g.check), F.mul(F.mul(lchk, a_n), F.load(nxt, g.b_inv[0]))), trans,
             AirCons{LSP_CONSTRAINT_TRANSITION, -1});
        push(F.sub(lchk, one), last, AirCons{LSP_CONSTRAINT_LAST_ROW, -1});
    } else {  // AirLookupConfig: air/src/lib.rs:57-114
        const AirView g = air_decode(LSP_AIR_LOOKUP, r);
        const V a_l = air_combo(F, loc, g.a, g.na, alpha, delta);
        const V lainv = F.load(loc, g.a_inv);
        push(F.sub(F.mul(a_l, lainv), one), always, AirCons{LSP_CONSTRAINT_A_INVERSE, -1});
        V lc = F.mul(F.load(loc, g.a_filter), lainv);
        V nc = F.mul(F.load(nxt, g.a_filter), F.load(nxt, g.a_inv));
        for (int32_t t = 0; t < g.ntab; ++t) {
            const V b_l = air_combo(F, loc, g.b + t * g.nbc, g.nbc, alpha, delta);
            const V lbinv = F.load(loc, g.b_inv[t]);
            push(F.sub(F.mul(b_l, lbinv), one), always, AirCons{LSP_CONSTRAINT_B_INVERSE, t});
            lc = F.sub(lc, F.mul(F.mul(F.load(loc, g.b_filter[t]), F.load(loc, g.occ[t])), lbinv));
            nc = F.sub(nc, F.mul(F.mul(F.load(nxt, g.b_filter[t]), F.load(nxt, g.occ[t])), F.load(nxt, g.b_inv[t])));
        }
        const V lchk = F.load(loc, g.check);
        push(F.sub(lchk, lc), first, AirCons{LSP_CONSTRAINT_FIRST_ROW, -1});
        push(F.sub(F.sub(F.load(nxt, g.check), lchk), nc), trans, AirCons{LSP_CONSTRAINT_TRANSITION, -1});
        push(lchk, last, AirCons{LSP_CONSTRAINT_LAST_ROW, -1});
    }
}

}  // namespace lsp
