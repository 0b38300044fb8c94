// Coset LDE drivers (the fused LDE pass, its coefficient and sub-coset forms,
// coset_dft / coset_idft) and the power and twist tables they cache in the
// context.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "host.hpp"
#include "prove_internal.hpp"

namespace lsp {

static void two_level(uint32_t bits, uint32_t& L1, uint32_t& L2) {
    L1 = (bits + 1) / 2;
    L2 = bits - L1;
}

// two-level power table of `base` covering exponents < 2^bits, in pool buffer `name`
// cached per (base, bits) in the context: the tables of one proof shape (the
// quotient and LDE domains, every FRI round's w^-1) are the same every proof
const Fr* pow_table(lsp_ctx* ctx, const std::string& name, const Fr& base, uint32_t bits, uint32_t& L1) {
    uint32_t L2;
    two_level(bits, L1, L2);
    char key[96];
    std::snprintf(key, sizeof key, "ptab_%u_%08x%08x%08x%08x%08x%08x%08x%08x", bits, base.v[7], base.v[6], base.v[5],
                  base.v[4], base.v[3], base.v[2], base.v[1], base.v[0]);
    auto it = ctx->ptabs.find(key);
    if (it != ctx->ptabs.end()) return it->second;
    Fr* tab = ctx->fbuf(key, (1ull << L1) + (1ull << L2));
    Fr* b = ctx->fbuf(name + "_base", 1);
    LSP_HIP(hipMemcpyAsync(b, &base, sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    LSP_HIP(launch_pow_tables(b, 1, L1, L2, nullptr, tab, ctx->stream));
    LSP_HIP(hipStreamSynchronize(ctx->stream));  // `base` is a host temporary
    ctx->ptabs[key] = tab;
    return tab;
}

Fr d2h_fr(lsp_ctx* ctx, const Fr* d) {
    Fr x;
    LSP_HIP(hipMemcpyAsync(&x, d, sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    LSP_HIP(hipStreamSynchronize(ctx->stream));
    return x;
}

// ----------------------------------------------------------------- LDE
// The twist tables of coset blocks [k0, k0 + nk) of an h x w LDE: coset k,
// column c has base s = shift_c * w_N^bitrev(k); coefficient i is scaled by
// s^i / h (s^i with div_h false: a transform of true coefficients).  Built
// once per (log h, cosets, shifts, div_h) and kept in the context.
struct TwistTables {
    const Fr* tabs;
    uint32_t L1, L2;
    bool shared;  // one table per coset (every column's shift is the same)
};
static TwistTables lde_twist(lsp_ctx* ctx, size_t h, size_t w, uint32_t added_bits, const Fr* shifts_host, uint32_t k0,
                             uint32_t nk, bool div_h = true) {
    const uint32_t logh = log2_exact(h);
    const uint32_t logN = logh + added_bits;
    hipStream_t st = ctx->stream;
    TwistTables T;
    T.shared = true;
    for (size_t c = 1; c < w; ++c) T.shared = T.shared && fr_eq(shifts_host[c], shifts_host[0]);
    const size_t per_coset = T.shared ? 1 : w;
    two_level(logh, T.L1, T.L2);
    const size_t per = (1ull << T.L1) + (1ull << T.L2);
    const size_t nb = (size_t)nk * per_coset;
    uint64_t hsh = 1469598103934665603ull;  // FNV-1a over the shifts' words
    for (size_t c = 0; c < per_coset; ++c)
        for (int i = 0; i < 8; ++i) hsh = (hsh ^ shifts_host[c].v[i]) * 1099511628211ull;
    char key[112];
    std::snprintf(key, sizeof key, "ldetw_%u_%u_%u_%u_%zu_%d_%016llx", logh, added_bits, k0, nk, per_coset,
                  div_h ? 1 : 0, (unsigned long long)hsh);
    auto it = ctx->ptabs.find(key);
    if (it != ctx->ptabs.end()) {
        T.tabs = it->second;
        return T;
    }
    const Fr wN = host_two_adic_generator(logN);
    const Fr hinv = div_h ? host_inv_cached(fr_from_u64(h)) : fr_one();
    std::vector<Fr> bases(2 * nb, hinv);  // nb bases, then nb scales (1/h or 1)
    for (uint32_t k = 0; k < nk; ++k) {
        const Fr ck = fr_pow_u64(wN, host_bitrev(k0 + k, added_bits));
        for (size_t c = 0; c < per_coset; ++c) bases[k * per_coset + c] = fr_mul(shifts_host[c], ck);
    }
    Fr* dbases = ctx->fbuf("lde_bases", 2 * nb);
    ctx->h2d_async("lde_bases_h", dbases, bases.data(), bases.size() * sizeof(Fr));
    const bool keep = ctx->ptabs.size() < 256;  // API callers with ever new shifts: a scratch table
    Fr* t = ctx->fbuf(keep ? key : "lde_tabs", per * nb);
    LSP_HIP(launch_pow_tables(dbases, nb, T.L1, T.L2, dbases + nb, t, st));
    LSP_HIP(launch_to_f29form(t, t, per * nb, st));  // the NTT multiplies by 29-bit-form factors
    if (keep) ctx->ptabs[key] = t;
    T.tabs = t;
    return T;
}

// The chained twist of the fused LDE pass (launch_lde's `ratio`): blocks
// k0 + bitrev_a(j), j < nk = 2^a, k0 a multiple of nk, have the shifts
// shift_c w_N^bitrev_b(k0) rho^j with rho = w_N^(2^b / nk), so the pass twists
// block 0 from its table and every later block by rho^row.  The two-level table
// of rho^i (29-bit form, cached in the context), or nullptr when the range is
// not such a run or LSP_NTT_CHAIN=0 (A/B).
static const Fr* chain_ratio(lsp_ctx* ctx, uint32_t logh, uint32_t added_bits, uint32_t k0, uint32_t nk) {
    static const bool on = [] {
        const char* e = std::getenv("LSP_NTT_CHAIN");
        return !(e && *e == '0');
    }();
    if (!on || logh == 0 || nk < 2 || (nk & (nk - 1)) != 0 || k0 % nk != 0 || nk > (1u << added_bits)) return nullptr;
    const uint32_t logN = logh + added_bits;
    const Fr rho = fr_pow_u64(host_two_adic_generator(logN), (1ull << added_bits) / nk);
    uint32_t L1, L2;
    two_level(logh, L1, L2);
    char key[112];
    std::snprintf(key, sizeof key, "ldechain_%u_%08x%08x%08x%08x%08x%08x%08x%08x", logh, rho.v[7], rho.v[6], rho.v[5],
                  rho.v[4], rho.v[3], rho.v[2], rho.v[1], rho.v[0]);
    auto it = ctx->ptabs.find(key);
    if (it != ctx->ptabs.end()) return it->second;
    Fr* tab = ctx->fbuf(key, (1ull << L1) + (1ull << L2));
    Fr* b = ctx->fbuf("ldechain_base", 1);
    LSP_HIP(hipMemcpyAsync(b, &rho, sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    LSP_HIP(launch_pow_tables(b, 1, L1, L2, nullptr, tab, ctx->stream));
    LSP_HIP(launch_to_f29form(tab, tab, (1ull << L1) + (1ull << L2), ctx->stream));
    LSP_HIP(hipStreamSynchronize(ctx->stream));  // `rho` is a host temporary
    ctx->ptabs[key] = tab;
    return tab;
}

// Coset blocks [k0, k0 + nk) of the bit-reversed LDE (nk = 0: all
// 2^added_bits): block k = rows k*h .. (k+1)*h - 1 of the full LDE, the
// evaluations on shift_c * w_N^bitrev(k) * H_h.  d_out receives nk blocks.
void lde_device(lsp_ctx* ctx, const Fr* d_in, size_t h, size_t w, uint32_t added_bits, const Fr* shifts_host,
                Fr* d_out, uint32_t k0, uint32_t nk) {
    const uint32_t logh = log2_exact(h);
    const uint32_t B = 1u << added_bits;
    if (nk == 0) nk = B;
    LSP_REQUIRE(k0 + nk <= B, LSP_E_ARG, "coset range outside the LDE");
    LSP_REQUIRE(logh + added_bits <= 47, LSP_E_SIZE, "LDE larger than the 2-adic subgroup");
    Fr* X = ctx->fbuf("lde_X", h * w);
    // with the chained twist the fused pass reads only block k0's table (the
    // later blocks multiply by rho^row), so only that one is built and cached
    const Fr* ratio = chain_ratio(ctx, logh, added_bits, k0, nk);
    const TwistTables T = lde_twist(ctx, h, w, added_bits, shifts_host, k0, ratio ? 1 : nk);
    LSP_HIP(launch_lde(d_in, X, d_out, w, logh, nk, ctx->twiddle29(logh, true), ctx->twiddle29(logh, false), T.tabs,
                       T.L1, T.L2, T.shared ? 0 : 1, ratio, ctx->stream));
}

// The same blocks from h * coefficients (natural order) at `coef`, laid out
// as `map` says -- the forward half, for ranks that split the inverse
void lde_coeffs_device(lsp_ctx* ctx, const Fr* coef, ColMap map, size_t h, size_t w, uint32_t added_bits,
                       const Fr* shifts_host, Fr* d_out, uint32_t k0, uint32_t nk, bool div_h) {
    const uint32_t logh = log2_exact(h);
    LSP_REQUIRE(k0 + nk <= (1u << added_bits) && logh >= 1, LSP_E_ARG, "coset range outside the LDE");
    const Fr* ratio = chain_ratio(ctx, logh, added_bits, k0, nk);  // (block k0's table only, as lde_device)
    const TwistTables T = lde_twist(ctx, h, w, added_bits, shifts_host, k0, ratio ? 1 : nk, div_h);
    LSP_HIP(launch_lde_coeffs(coef, map, d_out, w, logh, nk, ctx->twiddle29(logh, false), T.tabs, T.L1, T.L2,
                              T.shared ? 0 : 1, ratio, ctx->stream));
}

// TwoAdicSubgroupDft::coset_dft_batch ([EXT p3-dft]; dft_batch: shift 1): the
// h x w true coefficients at d_coef -> evaluations on shift H_h, stored
// bit-reversed (row j = p(shift w_h^bitrev(j)), Radix2DitParallel's
// Evaluations layout) -- the forward half of the LDE with one block and
// twist s^i instead of s^i / h
void coset_dft_device(lsp_ctx* ctx, const Fr* d_coef, size_t h, size_t w, const Fr& shift, Fr* d_out) {
    const uint32_t logh = log2_exact(h);
    LSP_REQUIRE(logh <= 40, LSP_E_SIZE, "transform too large");
    if (h == 1) {  // p(x) = c_0 everywhere
        if (d_out != d_coef)
            LSP_HIP(hipMemcpyAsync(d_out, d_coef, w * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
        return;
    }
    const std::vector<Fr> sh(w, shift);
    lde_coeffs_device(ctx, d_coef, ColMap::plain((uint32_t)w), h, w, 0, sh.data(), d_out, 0, 1, false);
}

// TwoAdicSubgroupDft::coset_idft_batch (idft_batch: shift 1): evaluations on
// shift H_h in natural row order -> the coefficients (natural order,
// canonical): the LDE's inverse half (h c_i), then c_i = X_i (1/h) shift^-i
void coset_idft_device(lsp_ctx* ctx, const Fr* d_evals, size_t h, size_t w, const Fr& shift, Fr* d_out) {
    const uint32_t logh = log2_exact(h);
    LSP_REQUIRE(logh <= 40, LSP_E_SIZE, "transform too large");
    LSP_REQUIRE(!fr_is_zero(fr_to_canonical(shift)), LSP_E_ARG, "coset shift must be nonzero");
    uint32_t L1, L2;
    two_level(logh, L1, L2);
    const size_t per = (1ull << L1) + (1ull << L2);
    Fr* tab = ctx->fbuf("idft_tab", per);
    Fr* b = ctx->fbuf("idft_tab_base", 2);
    const Fr base_scale[2] = {host_inv_cached(shift), host_inv_cached(fr_from_u64(h))};
    LSP_HIP(hipMemcpyAsync(b, base_scale, sizeof base_scale, hipMemcpyHostToDevice, ctx->stream));
    LSP_HIP(launch_pow_tables(b, 1, L1, L2, b + 1, tab, ctx->stream));
    LSP_HIP(launch_to_f29form(tab, tab, per, ctx->stream));
    const Fr* X = d_evals;  // h = 1: the value is the coefficient
    if (h > 1) {
        Fr* x = ctx->fbuf("idft_X", h * w);
        LSP_HIP(launch_intt(d_evals, ColMap::plain((uint32_t)w), x, w, logh, ctx->twiddle29(logh, true), ctx->stream));
        X = x;
    }
    LSP_HIP(launch_scale_coeffs(X, h, (uint32_t)w, tab, L1, d_out, ctx->stream));
    LSP_HIP(hipStreamSynchronize(ctx->stream));  // `base_scale` is a host temporary
}

// Block `blk` (S = N / 2^b rows, S < h) of the bit-reversed N-row LDE, when a
// proof has more ranks than cosets: the evaluations on the sub-coset
// c H_S, c = shift_c w_N^bitrev_b(blk).  The h coefficients of every column
// fold to S (c'_i = sum_t c_(i + t S) c^(t S), SURVEY 8(e) step 6 without a
// transpose), then one size-S coset NTT of the folded columns, which is
// lde_coeffs_device with the LDE seen as 2^b blocks of S rows.  The fold also
// divides by f = h / S, so the NTT's 1/S twist scale gives the 1/h the
// coefficients (h * c_i, as the inverse leaves them) need.
void subcoset_lde(lsp_ctx* ctx, const Fr* coef, ColMap map, size_t h, size_t w, uint32_t logN, uint32_t b,
                  uint32_t blk, const Fr* shifts_host, Fr* d_out, const std::string& tag) {
    const size_t S = (size_t)1 << (logN - b), f = h / S;
    LSP_REQUIRE(S < h && f <= 64 && S >= 2, LSP_E_ARG, "sub-coset outside 2 .. h/2 rows");
    const Fr cb = fr_pow_u64(host_two_adic_generator(logN), host_bitrev(blk, b));
    const Fr finv = host_inv_cached(fr_from_u64(f));
    std::vector<Fr> fac(w * f);
    for (size_t c = 0; c < w; ++c) {
        const Fr sigma = fr_pow_u64(fr_mul(shifts_host[c], cb), S);
        Fr x = finv;
        for (size_t t = 0; t < f; ++t) {
            fac[c * f + t] = x;
            x = fr_mul(x, sigma);
        }
    }
    Fr* dfac = ctx->fbuf(tag + "_fac", w * f);
    ctx->h2d_async(tag + "_fac_h", dfac, fac.data(), fac.size() * sizeof(Fr));
    LSP_HIP(launch_to_f29form(dfac, dfac, w * f, ctx->stream));
    Fr* folded = ctx->fbuf(tag + "_fold", S * w);
    LSP_HIP(launch_fold_subcoset(coef, map, h, S, (uint32_t)w, dfac, folded, ctx->stream));
    lde_coeffs_device(ctx, folded, ColMap::plain((uint32_t)w), S, w, b, shifts_host, d_out, blk, 1);
}

}  // namespace lsp
