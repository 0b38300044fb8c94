// csrc/witness_layout.hpp against its own documentation and against the
// descriptor's reader (air_walk.hpp's air_decode), with the host compiler
// alone: for na, nb in 1..4, nt, nbc in 1..3 and col0 in {0, 5}
//   - the named columns, in the documented order, are 0 .. width() - 1, each once
//   - the raw offsets tile 0 .. raw_cols() - 1 in the order a | b | a_filter | b_filter
//   - describe() writes desc_len() words, and decoding them gives the named
//     columns shifted by col0
// and the widths the documents quote.  Prints "N failure(s)"; exit status 0 iff N = 0.
#include <cstdio>
#include <vector>

#define __host__
#define __device__
#define __forceinline__ inline
#include "air_walk.hpp"
#include "witness_layout.hpp"

using namespace lsp;

static int failures = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            ++failures;                                       \
            std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                         \
            std::printf("\n");                                \
        }                                                     \
    } while (0)

static_assert(PermBlock{6, 6}.width() == 14, "the benchmark's permutation group");
static_assert(LookupBlock{3, 2, 3}.width() == 18, "the wide AIR's lookup");
static_assert(4 * LookupBlock{3, 2, 3}.width() + 8 * PermBlock{6, 6}.width() == 184, "the default wide shape");

// the ids are 0, 1, 2, ... in this order
static void check_sequence(const std::vector<size_t>& ids, size_t width, const char* what) {
    CHECK(ids.size() == width, "%s: %zu named columns, width %zu", what, ids.size(), width);
    for (size_t k = 0; k < ids.size(); ++k) CHECK(ids[k] == k, "%s: column %zu is named %zu", what, k, ids[k]);
}

// describe() into a guarded buffer: exactly desc_len() words, the config count left to the caller
template <class Block>
static std::vector<int32_t> described(const Block& blk, size_t col0) {
    const int32_t canary = 0x5ca1ab1e;
    std::vector<int32_t> d(blk.desc_len() + 1, canary);
    int32_t* end = blk.describe(col0, d.data());
    CHECK((size_t)(end - d.data()) == blk.desc_len(), "wrote %td words, desc_len %zu", end - d.data(), blk.desc_len());
    CHECK(d.back() == canary, "describe wrote past desc_len()");
    for (size_t k = 0; k + 1 < d.size(); ++k) CHECK(d[k] != canary, "word %zu not written", k);
    return d;
}

static void check_perm(uint32_t na, uint32_t nb, size_t col0) {
    const PermBlock blk{na, nb};
    std::vector<size_t> ids;
    for (uint32_t k = 0; k < na; ++k) ids.push_back(blk.a(k));
    for (uint32_t k = 0; k < nb; ++k) ids.push_back(blk.b(k));
    ids.push_back(blk.b_inv());
    ids.push_back(blk.check());
    check_sequence(ids, blk.width(), "permutation");
    CHECK(blk.raw_a() == 0 && blk.raw_b() == blk.raw_a() + na && blk.raw_cols() == blk.raw_b() + nb,
          "raw offsets %zu %zu of %zu", blk.raw_a(), blk.raw_b(), blk.raw_cols());

    const std::vector<int32_t> d = described(blk, col0);
    CHECK(d[0] == LSP_AIR_PERMUTATION, "type word %d", d[0]);
    AirWords r{d.data(), 1};
    const AirView g = air_decode(d[0], r);
    CHECK((size_t)r.p == blk.desc_len(), "decoded %d words of %zu", r.p, blk.desc_len());
    CHECK(g.na == (int32_t)na && g.nbc == (int32_t)nb && g.ntab == 1, "counts %d %d %d", g.na, g.nbc, g.ntab);
    for (uint32_t k = 0; k < na; ++k) CHECK(g.a[k] == (int32_t)(col0 + blk.a(k)), "a[%u] = %d", k, g.a[k]);
    for (uint32_t k = 0; k < nb; ++k) CHECK(g.b[k] == (int32_t)(col0 + blk.b(k)), "b[%u] = %d", k, g.b[k]);
    CHECK(g.b_inv[0] == (int32_t)(col0 + blk.b_inv()), "b_inv = %d", g.b_inv[0]);
    CHECK(g.check == (int32_t)(col0 + blk.check()), "check = %d", g.check);
}

static void check_lookup(uint32_t na, uint32_t nt, uint32_t nbc, size_t col0) {
    const LookupBlock blk{na, nt, nbc};
    std::vector<size_t> ids;
    for (uint32_t k = 0; k < na; ++k) ids.push_back(blk.a(k));
    for (uint32_t t = 0; t < nt; ++t)
        for (uint32_t c = 0; c < nbc; ++c) ids.push_back(blk.b(t, c));
    ids.push_back(blk.a_filter());
    for (uint32_t t = 0; t < nt; ++t) ids.push_back(blk.b_filter(t));
    ids.push_back(blk.a_inv());
    for (uint32_t t = 0; t < nt; ++t) ids.push_back(blk.b_inv(t));
    for (uint32_t t = 0; t < nt; ++t) ids.push_back(blk.mult(t));
    ids.push_back(blk.sum());
    check_sequence(ids, blk.width(), "lookup");
    CHECK(blk.raw_a() == 0 && blk.raw_b() == blk.raw_a() + na && blk.raw_a_filter() == blk.raw_b() + (size_t)nt * nbc &&
              blk.raw_b_filter() == blk.raw_a_filter() + 1 && blk.raw_cols() == blk.raw_b_filter() + nt,
          "raw offsets %zu %zu %zu %zu of %zu", blk.raw_a(), blk.raw_b(), blk.raw_a_filter(), blk.raw_b_filter(),
          blk.raw_cols());

    const std::vector<int32_t> d = described(blk, col0);
    CHECK(d[0] == LSP_AIR_LOOKUP, "type word %d", d[0]);
    AirWords r{d.data(), 1};
    const AirView g = air_decode(d[0], r);
    CHECK((size_t)r.p == blk.desc_len(), "decoded %d words of %zu", r.p, blk.desc_len());
    CHECK(g.na == (int32_t)na && g.ntab == (int32_t)nt && g.nbc == (int32_t)nbc, "counts %d %d %d", g.na, g.ntab, g.nbc);
    for (uint32_t k = 0; k < na; ++k) CHECK(g.a[k] == (int32_t)(col0 + blk.a(k)), "a[%u] = %d", k, g.a[k]);
    for (uint32_t t = 0; t < nt; ++t) {
        for (uint32_t c = 0; c < nbc; ++c)
            CHECK(g.b[t * nbc + c] == (int32_t)(col0 + blk.b(t, c)), "b[%u][%u] = %d", t, c, g.b[t * nbc + c]);
        CHECK(g.b_filter[t] == (int32_t)(col0 + blk.b_filter(t)), "b_filter[%u] = %d", t, g.b_filter[t]);
        CHECK(g.b_inv[t] == (int32_t)(col0 + blk.b_inv(t)), "b_inv[%u] = %d", t, g.b_inv[t]);
        CHECK(g.occ[t] == (int32_t)(col0 + blk.mult(t)), "mult[%u] = %d", t, g.occ[t]);
    }
    CHECK(g.a_filter == (int32_t)(col0 + blk.a_filter()), "a_filter = %d", g.a_filter);
    CHECK(g.a_inv == (int32_t)(col0 + blk.a_inv()), "a_inv = %d", g.a_inv);
    CHECK(g.check == (int32_t)(col0 + blk.sum()), "sum = %d", g.check);
}

int main() {
    int cases = 0;
    for (size_t col0 : {(size_t)0, (size_t)5})
        for (uint32_t na = 1; na <= 4; ++na) {
            for (uint32_t nb = 1; nb <= 4; ++nb, ++cases) check_perm(na, nb, col0);
            for (uint32_t nt = 1; nt <= 3; ++nt)
                for (uint32_t nbc = 1; nbc <= 3; ++nbc, ++cases) check_lookup(na, nt, nbc, col0);
        }
    std::printf("%d blocks, %d failure(s)\n", cases, failures);
    return failures ? 1 : 0;
}
