// Witness generation -- the reference's `trace` crate semantics
// (RawPermutationTrace::get_trace, trace/src/permutation.rs:24-93;
// RawLookupTrace::get_trace, trace/src/lookup.rs:46-176; RawTrace::push_traces /
// get_trace, trace/src/lib.rs:62-106) -- on the host and on the device.  Both
// take a block's raw columns column-major and write its rows at
// out + i * ostride; which column holds what is witness_layout.hpp's.
//
// The host functions build the synthetic traces (the wide-AIR workload of
// SURVEY 8(d) C3, the stand-in for the missing zkevm.bin, and the permutation
// benchmark trace).  The witness path's extern "C" entry points (include/lsp.h)
// are at the end: witness blocks (F1), CBOR raw traces (F4), the generators.
#include <cstring>
#include <unordered_map>

#include "capi_internal.hpp"
#include "splitmix.hpp"

namespace lsp {
namespace {
// The two ways a block fails, with the reference's words: it panics in
// Field::inverse of zero, and asserts the check column's last row
const char* const INVERT_ZERO = "tried to invert zero (row combination + delta = 0)";
void require_last_row(bool ok, const char* want) {
    LSP_REQUIRE(ok, LSP_E_STATE,
                std::string("failed to check constrain: check column should be ") + want + " on the last row");
}

struct FrHash {
    size_t operator()(const Fr& x) const {
        uint64_t h = 0xcbf29ce484222325ull;
        for (int i = 0; i < 8; ++i) h = (h ^ x.v[i]) * 0x100000001b3ull;
        return (size_t)h;
    }
};
struct FrEq {
    bool operator()(const Fr& a, const Fr& b) const { return fr_eq(a, b); }
};

// v[i] <- 1 / v[i], one field inversion for all of them
void batch_inv(Fr* v, size_t n) {
    std::vector<Fr> pre(n);
    Fr acc = fr_one();
    for (size_t i = 0; i < n; ++i) {
        pre[i] = acc;
        acc = fr_mul(acc, v[i]);
    }
    LSP_REQUIRE(!fr_is_zero(acc), LSP_E_STATE, INVERT_ZERO);
    Fr inv = fr_inv(acc);
    for (size_t i = n; i-- > 0;) {
        const Fr t = fr_mul(inv, pre[i]);
        inv = fr_mul(inv, v[i]);
        v[i] = t;
    }
}
}  // namespace

// RawPermutationTrace::get_trace on the host.  b_row (optional): B's row i is
// row b_row[i] of b's columns, so a B that is a row shuffle of A (b = a) needs
// no copy.  Two n-vectors of scratch.
static void witness_permutation_host(const Fr* a, uint32_t na, const Fr* b, uint32_t nb, size_t n, const Fr& alpha,
                                     const Fr& delta, Fr* out, size_t ostride, const size_t* b_row = nullptr) {
    const PermBlock blk{na, nb};
    std::vector<Fr> binv(n);
    for (size_t i = 0; i < n; ++i)
        binv[i] = fr_add(put_combo(b, nb, n, b_row ? b_row[i] : i, alpha, out + i * ostride,
                                   [&](uint32_t k) { return blk.b(k); }),
                         delta);
    batch_inv(binv.data(), n);
    Fr prev = fr_one();
    for (size_t i = 0; i < n; ++i) {
        Fr* row = out + i * ostride;
        const Fr al = fr_add(put_combo(a, na, n, i, alpha, row, [&](uint32_t k) { return blk.a(k); }), delta);
        row[blk.b_inv()] = binv[i];
        prev = fr_mul(fr_mul(prev, al), binv[i]);
        row[blk.check()] = prev;
    }
    require_last_row(fr_eq(prev, fr_one()), "1");
}

// RawLookupTrace::get_trace on the host
static void witness_lookup_host(const Fr* a, uint32_t na, const Fr* b, uint32_t nt, uint32_t nbc, const Fr* afil,
                                const Fr* bfil, size_t n, const Fr& alpha, const Fr& delta, Fr* out,
                                size_t ostride) {
    const LookupBlock blk{na, nt, nbc};
    const size_t m = n * (1 + (size_t)nt);
    std::vector<Fr> comb(m), inv(m);  // [A | table 0 | table 1 | ...], as on the device
    std::unordered_map<Fr, uint64_t, FrHash, FrEq> occ;  // enabled A rows per combination
    for (size_t i = 0; i < n; ++i) {
        Fr* row = out + i * ostride;
        comb[i] = put_combo(a, na, n, i, alpha, row, [&](uint32_t k) { return blk.a(k); });
        if (!fr_is_zero(afil[i])) occ[comb[i]] += 1;
        row[blk.a_filter()] = afil[i];
        for (uint32_t t = 0; t < nt; ++t) {
            comb[(1 + (size_t)t) * n + i] =
                put_combo(b + (size_t)t * nbc * n, nbc, n, i, alpha, row, [&](uint32_t k) { return blk.b(t, k); });
            row[blk.b_filter(t)] = bfil[(size_t)t * n + i];
        }
    }
    for (size_t r = 0; r < m; ++r) inv[r] = fr_add(comb[r], delta);
    batch_inv(inv.data(), m);
    // the first enabled B entry of a combination, in (row, table) order, takes its count
    Fr s = fr_zero();
    for (size_t i = 0; i < n; ++i) {
        Fr* row = out + i * ostride;
        row[blk.a_inv()] = inv[i];
        if (!fr_is_zero(afil[i])) s = fr_add(s, inv[i]);
        for (uint32_t t = 0; t < nt; ++t) {
            const size_t r = (1 + (size_t)t) * n + i;
            Fr o = fr_zero();
            auto it = occ.find(comb[r]);
            if (it != occ.end() && !fr_is_zero(bfil[(size_t)t * n + i])) {
                o = fr_from_u64(it->second);
                s = fr_sub(s, fr_mul(inv[r], o));
                occ.erase(it);
            }
            row[blk.b_inv(t)] = inv[r];
            row[blk.mult(t)] = o;
        }
        row[blk.sum()] = s;
    }
    require_last_row(fr_is_zero(s), "0");
}

// The wide synthetic trace: nlookup LogUp lookups of shape lk
// followed by nperm permutation groups of shape pm, in RawTrace's order
// (lookups first, trace/src/lib.rs:81-89), each block at the columns already
// pushed.  rows: 2^log_n x width; desc: the AIR descriptor.  Deterministic in
// `seed`: per lookup the tables are drawn, then each A row's (table, row)
// pair; per permutation A, then the Fisher-Yates shuffle that makes B.
static void gen_wide_trace(uint64_t seed, uint32_t log_n, uint32_t nlookup, LookupBlock lk, uint32_t nperm,
                           PermBlock pm, const Fr& alpha, const Fr& delta, Fr* rows, size_t width, int32_t* desc) {
    const size_t n = (size_t)1 << log_n;
    SplitMix64 g{seed ^ 0x57494445ull};  // "WIDE"
    *desc++ = (int32_t)(nlookup + nperm);
    size_t col0 = 0;
    std::vector<Fr> raw;
    for (uint32_t l = 0; l < nlookup; ++l) {
        raw.assign(lk.raw_cols() * n, fr_one());  // the filters stay 1: every row enabled
        Fr* a = raw.data() + lk.raw_a() * n;
        Fr* b = raw.data() + lk.raw_b() * n;
        for (size_t x = 0; x < (size_t)lk.nt * lk.nbc * n; ++x) b[x] = g.fr();
        for (size_t i = 0; i < n; ++i) {
            const size_t t = (size_t)g.below(lk.nt), j = (size_t)g.below(n);
            for (uint32_t c = 0; c < lk.na; ++c) a[c * n + i] = b[(t * lk.nbc + c) * n + j];
        }
        witness_lookup_host(a, lk.na, b, lk.nt, lk.nbc, raw.data() + lk.raw_a_filter() * n,
                            raw.data() + lk.raw_b_filter() * n, n, alpha, delta, rows + col0, width);
        desc = lk.describe(col0, desc);
        col0 += lk.width();
    }
    std::vector<size_t> perm(n);
    for (uint32_t p = 0; p < nperm; ++p) {
        raw.resize(pm.raw_cols() * n);
        Fr* a = raw.data() + pm.raw_a() * n;
        Fr* b = raw.data() + pm.raw_b() * n;
        for (size_t x = 0; x < (size_t)pm.na * n; ++x) a[x] = g.fr();
        for (size_t i = 0; i < n; ++i) perm[i] = i;
        for (size_t i = n - 1; i > 0; --i) std::swap(perm[i], perm[(size_t)g.below(i + 1)]);
        // B column by column: the gather stays within one column (a cache's
        // worth) at a time, where a row map over all columns misses it
        for (uint32_t c = 0; c < pm.nb; ++c)
            for (size_t i = 0; i < n; ++i) b[c * n + i] = a[c * n + perm[i]];
        witness_permutation_host(a, pm.na, b, pm.nb, n, alpha, delta, rows + col0, width);
        desc = pm.describe(col0, desc);
        col0 += pm.width();
    }
}

// ------------------------------------------------- device witness (F1)
namespace {
// The check column's last row and the zero-denominator flag come back in one
// copy: the column's buffer has one element more than rows, and the row
// kernels set that element's first word when a row combination + delta is 0.
// The reference panics there (Field::inverse of zero); the batch inverse maps
// 0 to 0, which would otherwise pass for a finished witness.
uint32_t* clear_zero_flag(Fr* col, size_t n, hipStream_t st) {
    LSP_HIP(hipMemsetAsync(col + n, 0, sizeof(Fr), st));
    return reinterpret_cast<uint32_t*>(col + n);
}
Fr fetch_last_row(const Fr* col, size_t n, hipStream_t st) {
    Fr tail[2];
    LSP_HIP(hipMemcpyAsync(tail, col + n - 1, sizeof tail, hipMemcpyDeviceToHost, st));
    LSP_HIP(hipStreamSynchronize(st));
    LSP_REQUIRE(tail[1].v[0] == 0, LSP_E_STATE, INVERT_ZERO);
    return tail[0];
}
}  // namespace
// RawPermutationTrace::get_trace on the device (the check column: prefix
// product of (a_comb + delta) / (b_comb + delta), must end at 1)
void witness_permutation_device(lsp_ctx* ctx, const Fr* a, uint32_t na, const Fr* b, uint32_t nb, size_t n,
                                const Fr& alpha, const Fr& delta, Fr* out, size_t ostride) {
    const PermBlock blk{na, nb};
    hipStream_t st = ctx->stream;
    Fr* al = ctx->fbuf("wit_al", n);
    Fr* bl = ctx->fbuf("wit_bl", n);
    Fr* binv = ctx->fbuf("wit_binv", n);
    Fr* chk = ctx->fbuf("wit_chk", n + 1);
    const size_t sb = witness_scratch_bytes(n, 0);
    void* scratch = ctx->buf("wit_scratch", sb);
    uint32_t* zflag = clear_zero_flag(chk, n, st);
    LSP_HIP(launch_perm_rows(a, b, blk, n, alpha, delta, out, ostride, al, bl, zflag, st));
    LSP_HIP(launch_batch_inverse(bl, binv, n, st, ctx->bi_scratch(n)));
    LSP_HIP(launch_mul_vec(al, binv, n, al, st));
    LSP_HIP(launch_fr_scan(al, chk, n, true, scratch, sb, st));
    LSP_HIP(launch_put_col(binv, n, out, ostride, blk.b_inv(), st));
    LSP_HIP(launch_put_col(chk, n, out, ostride, blk.check(), st));
    require_last_row(fr_eq(fetch_last_row(chk, n, st), fr_one()), "1");
}

// RawLookupTrace::get_trace on the device (the sum column: prefix sum of the LogUp terms, must end at 0)
void witness_lookup_device(lsp_ctx* ctx, const Fr* a, uint32_t na, const Fr* b, uint32_t nt, uint32_t nbc,
                           const Fr* afil, const Fr* bfil, size_t n, const Fr& alpha, const Fr& delta, Fr* out,
                           size_t ostride) {
    const LookupBlock blk{na, nt, nbc};
    hipStream_t st = ctx->stream;
    const size_t m = n * (1 + (size_t)nt);
    Fr* comb = ctx->fbuf("wit_comb", m);
    Fr* den = ctx->fbuf("wit_den", m);
    Fr* inv = ctx->fbuf("wit_inv", m);
    uint32_t* occ = (uint32_t*)ctx->buf("wit_occ", std::max<size_t>(1, n * nt) * sizeof(uint32_t));
    Fr* term = ctx->fbuf("wit_term", n);
    Fr* psum = ctx->fbuf("wit_psum", n + 1);
    const size_t sb = witness_scratch_bytes(n, nt);
    void* scratch = ctx->buf("wit_scratch", sb);
    uint32_t* zflag = clear_zero_flag(psum, n, st);
    LSP_HIP(launch_lookup_rows(a, b, blk, afil, bfil, n, alpha, delta, out, ostride, comb, den, zflag, st));
    LSP_HIP(launch_batch_inverse(den, inv, m, st, ctx->bi_scratch(m)));
    LSP_HIP(launch_lookup_occurrences(comb, n, nt, afil, bfil, occ, scratch, sb, st));
    LSP_HIP(launch_lookup_terms(inv, occ, afil, n, blk, out, ostride, term, st));
    LSP_HIP(launch_fr_scan(term, psum, n, false, scratch, sb, st));
    LSP_HIP(launch_put_col(psum, n, out, ostride, blk.sum(), st));
    require_last_row(fr_is_zero(fetch_last_row(psum, n, st)), "0");
}
}  // namespace lsp

using namespace lsp;

namespace {
// the block's rows: straight into a device trace, or via a scratch block and a
// strided copy into a host trace
template <class F>
void witness_block(lsp_ctx* ctx, lsp_fr* trace, size_t n, size_t trace_w, size_t col0, size_t bw, int mem, F&& fill) {
    LSP_REQUIRE(trace && col0 + bw <= trace_w, LSP_E_ARG, "witness block outside the trace width");
    if (mem == LSP_MEM_DEVICE) {
        fill(reinterpret_cast<Fr*>(trace) + col0, trace_w);
        return;
    }
    Fr* blk = ctx->fbuf("wit_block", n * bw);
    fill(blk, bw);
    LSP_HIP(hipMemcpy2DAsync(reinterpret_cast<Fr*>(trace) + col0, trace_w * sizeof(Fr), blk, bw * sizeof(Fr),
                             bw * sizeof(Fr), n, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
}
}  // namespace

extern "C" {

// ------------------------------------------------- witness generation (F1)
int lsp_witness_permutation(lsp_ctx* ctx, const lsp_fr* a, uint32_t na, const lsp_fr* b, uint32_t nb, size_t n,
                            const lsp_fr* alpha, const lsp_fr* delta, lsp_fr* trace, size_t trace_w, size_t col0,
                            int mem) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && alpha && delta && na >= 1 && nb >= 1 && n >= 1, LSP_E_ARG, "bad witness arguments");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        const Fr* da = dev_in(ctx, a, (size_t)na * n, mem, "wit_a");
        const Fr* db = dev_in(ctx, b, (size_t)nb * n, mem, "wit_b");
        const Fr al = to_fr(*alpha), de = to_fr(*delta);
        witness_block(ctx, trace, n, trace_w, col0, PermBlock{na, nb}.width(), mem, [&](Fr* out, size_t stride) {
            witness_permutation_device(ctx, da, na, db, nb, n, al, de, out, stride);
        });
    });
}

int lsp_witness_lookup(lsp_ctx* ctx, const lsp_fr* a, uint32_t na, const lsp_fr* b, uint32_t ntables, uint32_t nbc,
                       const lsp_fr* a_filter, const lsp_fr* b_filter, size_t n, const lsp_fr* alpha,
                       const lsp_fr* delta, lsp_fr* trace, size_t trace_w, size_t col0, int mem) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && alpha && delta && na >= 1 && ntables >= 1 && nbc >= 1 && n >= 1, LSP_E_ARG,
                    "bad witness arguments");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        const Fr* da = dev_in(ctx, a, (size_t)na * n, mem, "wit_a");
        const Fr* db = dev_in(ctx, b, (size_t)ntables * nbc * n, mem, "wit_b");
        const Fr* daf = dev_in(ctx, a_filter, n, mem, "wit_af");
        const Fr* dbf = dev_in(ctx, b_filter, (size_t)ntables * n, mem, "wit_bf");
        const Fr al = to_fr(*alpha), de = to_fr(*delta);
        witness_block(ctx, trace, n, trace_w, col0, LookupBlock{na, ntables, nbc}.width(), mem,
                      [&](Fr* out, size_t stride) {
                          witness_lookup_device(ctx, da, na, db, ntables, nbc, daf, dbf, n, al, de, out, stride);
                      });
    });
}

// ------------------------------------------------------ trace input (F4)
int lsp_raw_trace_parse(const uint8_t* cbor, size_t len, lsp_raw_trace** out) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(cbor && out, LSP_E_ARG, "null input");
        *out = parse_raw_trace(cbor, len);
    });
}

int lsp_raw_trace_shape(const lsp_raw_trace* t, int* kind, uint32_t* na, uint32_t* ntables, uint32_t* nbc,
                        size_t* max_height, size_t* width) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(t, LSP_E_ARG, "null trace");
        size_t h, w;
        raw_trace_shape(*t, h, w);
        if (kind) *kind = t->kind;
        if (na) *na = (uint32_t)t->a.size();
        if (ntables) *ntables = t->ntables;
        if (nbc) *nbc = t->nbc;
        if (max_height) *max_height = h;
        if (width) *width = w;
    });
}

int lsp_raw_trace_columns(const lsp_raw_trace* t, size_t height, lsp_fr* out, size_t cap, size_t* n) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(t && n, LSP_E_ARG, "null argument");
        const std::vector<Fr> cols = raw_trace_columns(*t, height);
        *n = cols.size();
        if (out) {
            LSP_REQUIRE(cap >= cols.size(), LSP_E_ARG, "buffer too small");
            std::memcpy(out, cols.data(), cols.size() * sizeof(Fr));
        }
    });
}

int lsp_raw_trace_push(lsp_ctx* ctx, const lsp_raw_trace* t, size_t height, const lsp_fr* alpha, const lsp_fr* delta,
                       lsp_fr* trace, size_t trace_w, size_t col0, int mem) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && t && alpha && delta && height >= 1, LSP_E_ARG, "bad raw trace push arguments");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        const std::vector<Fr> cols = raw_trace_columns(*t, height);  // RawTrace resize: zero words
        Fr* d = ctx->fbuf("raw_cols", cols.size());
        LSP_HIP(hipMemcpyAsync(d, cols.data(), cols.size() * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        const Fr al = to_fr(*alpha), de = to_fr(*delta);
        if (t->kind == LSP_AIR_PERMUTATION) {
            const PermBlock blk = t->perm();
            witness_block(ctx, trace, height, trace_w, col0, blk.width(), mem, [&](Fr* out, size_t stride) {
                witness_permutation_device(ctx, d + blk.raw_a() * height, blk.na, d + blk.raw_b() * height, blk.nb,
                                           height, al, de, out, stride);
            });
        } else {
            const LookupBlock blk = t->lookup();
            witness_block(ctx, trace, height, trace_w, col0, blk.width(), mem, [&](Fr* out, size_t stride) {
                witness_lookup_device(ctx, d + blk.raw_a() * height, blk.na, d + blk.raw_b() * height, blk.nt, blk.nbc,
                                      d + blk.raw_a_filter() * height, d + blk.raw_b_filter() * height, height, al,
                                      de, out, stride);
            });
        }
        ctx->sync();  // `cols` must outlive the upload
    });
}

int lsp_raw_trace_free(lsp_raw_trace* t) {
    delete t;
    return LSP_OK;
}

// ------------------------------------------------- synthetic traces
int lsp_gen_permutation_trace_device(lsp_ctx* ctx, uint64_t seed, uint32_t log_n, uint32_t ncols,
                                     const lsp_fr* alpha, const lsp_fr* delta, lsp_fr* trace) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && alpha && delta && trace && ncols >= 1 && log_n >= 1 && log_n <= 30, LSP_E_ARG,
                    "bad device trace-generator arguments");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        const size_t n = (size_t)1 << log_n;
        Fr* a = ctx->fbuf("gen_a", (size_t)ncols * n);
        Fr* b = ctx->fbuf("gen_b", (size_t)ncols * n);
        // the row bijection i -> (mul i + add) mod n: mul odd, both from the seed
        const uint64_t mul = ((seed * 0xD1B54A32D192ED03ull) ^ 0x5851F42D4C957F2Dull) | 1u;
        const uint64_t add = seed * 0xA24BAED4963EE407ull + 0x9FB21C651E98DF25ull;
        LSP_HIP(launch_gen_raw_perm(seed, n, ncols, mul, add, a, b, ctx->stream));
        witness_permutation_device(ctx, a, ncols, b, ncols, n, to_fr(*alpha), to_fr(*delta), (Fr*)trace,
                                   PermBlock{ncols, ncols}.width());
        ctx->release("gen_");
        ctx->release("wit_");
    });
}

// Host memory beyond the caller's rows: the ncols x n raw values of A, the row
// map that makes B of them, and witness_permutation_host's two n-vectors
int lsp_gen_permutation_trace(uint64_t seed, uint32_t log_n, uint32_t ncols, const lsp_fr* alpha,
                              const lsp_fr* delta, int small_values, lsp_fr* rows) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(alpha && delta && rows && ncols >= 1 && log_n >= 1 && log_n <= 30, LSP_E_ARG,
                    "bad trace arguments");
        const size_t n = (size_t)1 << log_n;
        SplitMix64 g{seed ^ 0x5452414345ull};  // "TRACE"
        std::vector<Fr> a((size_t)ncols * n);
        for (auto& x : a) x = small_values ? fr_from_u64(g.next() & 0xFFFFFFFFull) : g.fr();
        std::vector<size_t> perm(n);
        for (size_t i = 0; i < n; ++i) perm[i] = i;
        for (size_t i = n - 1; i > 0; --i) std::swap(perm[i], perm[g.below(i + 1)]);
        witness_permutation_host(a.data(), ncols, a.data(), ncols, n, to_fr(*alpha), to_fr(*delta),
                                 reinterpret_cast<Fr*>(rows), PermBlock{ncols, ncols}.width(), perm.data());
    });
}

int lsp_gen_wide_trace(uint64_t seed, uint32_t log_n, uint32_t nlookup, uint32_t na, uint32_t ntab, uint32_t nperm,
                       uint32_t pcols, const lsp_fr* alpha, const lsp_fr* delta, lsp_fr* rows_out, size_t rows_cap,
                       int32_t* air_out, size_t air_cap, size_t* width_out, size_t* air_len_out) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(alpha && delta && width_out && air_len_out && log_n >= 1 && log_n <= 26 &&
                        (nlookup == 0 || (na >= 1 && ntab >= 1)) && (nperm == 0 || pcols >= 1) &&
                        nlookup + nperm >= 1,
                    LSP_E_ARG, "bad wide-trace arguments");
        // sizes first (cheap): A of na columns drawn from ntab tables of na columns each
        const LookupBlock lk{na, ntab, na};
        const PermBlock pm{pcols, pcols};
        const size_t w = nlookup * lk.width() + nperm * pm.width();
        const size_t dl = 1 + nlookup * lk.desc_len() + nperm * pm.desc_len();
        *width_out = w;
        *air_len_out = dl;
        if (!rows_out) return;
        LSP_REQUIRE(rows_cap >= ((size_t)1 << log_n) * w && air_out && air_cap >= dl, LSP_E_ARG,
                    "output buffers too small");
        gen_wide_trace(seed, log_n, nlookup, lk, nperm, pm, to_fr(*alpha), to_fr(*delta),
                       reinterpret_cast<Fr*>(rows_out), w, air_out);
    });
}

}  // extern "C"
