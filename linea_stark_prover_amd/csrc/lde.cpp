// Coset LDE drivers: one transform request (lde) with coset_dft / coset_idft,
// the inverse half and the sub-coset form built on it, and the power, twist
// and twiddle tables they keep in the context (lsp_ctx::table).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "host.hpp"
#include "prove_internal.hpp"

namespace lsp {

// a two-level table covering exponents < 2^bits: 2^L1 low powers, 2^L2 high ones
static size_t two_level(uint32_t bits, uint32_t& L1, uint32_t& L2) {
    L1 = (bits + 1) / 2;
    L2 = bits - L1;
    return ((size_t)1 << L1) + ((size_t)1 << L2);
}

// the cache key of a table that one field element identifies
static std::string fr_key(const char* what, uint32_t bits, const Fr& x) {
    char key[112];
    std::snprintf(key, sizeof key, "%s_%u_%08x%08x%08x%08x%08x%08x%08x%08x", what, bits, x.v[7], x.v[6], x.v[5], x.v[4],
                  x.v[3], x.v[2], x.v[1], x.v[0]);
    return key;
}

// The fill of a table of nb two-level power tables (launch_pow_tables) from
// nb host bases -- with `scaled`, followed by the nb scales of the upper
// levels; f29: in the 29-bit Montgomery form the NTT multiplies by
static std::function<void(Fr*)> pow_fill(lsp_ctx* ctx, const Fr* bases, size_t nb, bool scaled, uint32_t L1,
                                         uint32_t L2, bool f29) {
    return [=](Fr* tab) {
        const size_t nh = scaled ? 2 * nb : nb;
        Fr* d = ctx->fbuf("tab_bases", nh);
        ctx->h2d_async("tab_bases_h", d, bases, nh * sizeof(Fr));
        LSP_HIP(launch_pow_tables(d, nb, L1, L2, scaled ? d + nb : nullptr, tab, ctx->stream));
        if (f29) LSP_HIP(launch_to_f29form(tab, tab, nb * (((size_t)1 << L1) + ((size_t)1 << L2)), ctx->stream));
    };
}

// two-level power table of `base` covering exponents < 2^bits, cached per
// (base, bits) in the context: the tables of one proof shape (the quotient and
// LDE domains, every FRI round's w^-1) are the same every proof
const Fr* pow_table(lsp_ctx* ctx, const Fr& base, uint32_t bits, uint32_t& L1) {
    uint32_t L2;
    const size_t per = two_level(bits, L1, L2);
    return ctx->table(fr_key("ptab", bits, base), per, pow_fill(ctx, &base, 1, false, L1, L2, false));
}

Fr d2h_fr(lsp_ctx* ctx, const Fr* d) {
    Fr x;
    LSP_HIP(hipMemcpyAsync(&x, d, sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    LSP_HIP(hipStreamSynchronize(ctx->stream));
    return x;
}

}  // namespace lsp

const uint4* lsp_ctx::twiddle29(uint32_t logH, bool inverse) {
    using namespace lsp;
    char key[32];
    std::snprintf(key, sizeof key, "tw29_%u_%d", logH, inverse ? 1 : 0);
    const size_t half = logH ? (size_t(1) << (logH - 1)) : 1, slots = logH ? (size_t(1) << logH) - 1 : 1;
    const Fr* t = table(key, (slots * 3 * sizeof(uint4) + sizeof(Fr) - 1) / sizeof(Fr), [&](Fr* out) {
        Fr w = host_two_adic_generator(logH);
        if (inverse) w = fr_inv(w);
        uint32_t L1, L2;
        Fr* tab = fbuf("tw_tab_tmp", two_level(logH ? logH - 1 : 0, L1, L2));
        pow_fill(this, &w, 1, false, L1, L2, false)(tab);
        Fr* pw = fbuf("tw_pow_tmp", half);
        LSP_HIP(launch_powers(tab, L1, half, pw, stream));
        LSP_HIP(launch_stage_twiddles(pw, logH, reinterpret_cast<uint4*>(out), stream));
    });
    return reinterpret_cast<const uint4*>(t);
}

namespace lsp {

// ----------------------------------------------------------------- LDE
// The twist tables of coset blocks [k0, k0 + nk) of an h x w LDE: coset k,
// column c has base s = shift_c * w_N^bitrev(k); coefficient i is scaled by
// s^i / h (s^i with div_h false: a transform of true coefficients).  Built
// once per (log h, cosets, shifts, div_h) and kept in the context; API callers
// with ever new shifts end up with a scratch table.
struct TwistTables {
    const Fr* tabs;
    uint32_t L1, L2;
    bool shared;  // one table per coset (every column's shift is the same)
};
static TwistTables lde_twist(lsp_ctx* ctx, size_t h, size_t w, uint32_t added_bits, const Fr* shifts_host, uint32_t k0,
                             uint32_t nk, bool div_h) {
    const uint32_t logh = log2_exact(h);
    TwistTables T;
    T.shared = true;
    for (size_t c = 1; c < w; ++c) T.shared = T.shared && fr_eq(shifts_host[c], shifts_host[0]);
    const size_t per_coset = T.shared ? 1 : w;
    const size_t per = two_level(logh, T.L1, T.L2);
    const size_t nb = (size_t)nk * per_coset;
    uint64_t hsh = 1469598103934665603ull;  // FNV-1a over the shifts' words
    for (size_t c = 0; c < per_coset; ++c)
        for (int i = 0; i < 8; ++i) hsh = (hsh ^ shifts_host[c].v[i]) * 1099511628211ull;
    char key[112];
    std::snprintf(key, sizeof key, "ldetw_%u_%u_%u_%u_%zu_%d_%016llx", logh, added_bits, k0, nk, per_coset,
                  div_h ? 1 : 0, (unsigned long long)hsh);
    T.tabs = ctx->table(
        key, per * nb,
        [&](Fr* tab) {
            const Fr wN = host_two_adic_generator(logh + added_bits);
            const Fr hinv = div_h ? host_inv_cached(fr_from_u64(h)) : fr_one();
            std::vector<Fr> bases(2 * nb, hinv);  // nb bases, then nb scales (1/h or 1)
            for (uint32_t k = 0; k < nk; ++k) {
                const Fr ck = fr_pow_u64(wN, host_bitrev(k0 + k, added_bits));
                for (size_t c = 0; c < per_coset; ++c) bases[k * per_coset + c] = fr_mul(shifts_host[c], ck);
            }
            pow_fill(ctx, bases.data(), nb, true, T.L1, T.L2, true)(tab);
        },
        "lde_tabs");
    return T;
}

// The chained twist of the fused LDE pass (NttLaunch::ratio): blocks
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
    const Fr rho = fr_pow_u64(host_two_adic_generator(logh + added_bits), (1ull << added_bits) / nk);
    uint32_t L1, L2;
    const size_t per = two_level(logh, L1, L2);
    return ctx->table(fr_key("ldechain", logh, rho), per, pow_fill(ctx, &rho, 1, false, L1, L2, true));
}

void lde(lsp_ctx* ctx, const LdeRequest& r) {
    const uint32_t logh = log2_exact(r.h);
    const uint32_t B = 1u << r.added_bits, nk = r.nk ? r.nk : B;
    LSP_REQUIRE(r.k0 + nk <= B, LSP_E_ARG, "coset range outside the LDE");
    LSP_REQUIRE(logh + r.added_bits <= 47, LSP_E_SIZE, "LDE larger than the 2-adic subgroup");
    NttLaunch a{.what = r.coeffs ? LDE_FWD : LDE_FULL, .src = r.src, .map = r.map,
                .scratch = r.coeffs ? nullptr : ctx->fbuf("lde_X", r.h * r.w), .out = r.out, .w = r.w, .logh = logh,
                .ncosets = nk};
    if (logh) {  // (h = 1 needs no table: launch_ntt)
        // with the chained twist the fused pass reads only block k0's table (the
        // later blocks multiply by rho^row), so only that one is built and cached
        a.ratio = chain_ratio(ctx, logh, r.added_bits, r.k0, nk);
        const TwistTables T = lde_twist(ctx, r.h, r.w, r.added_bits, r.shifts, r.k0, a.ratio ? 1 : nk, r.div_h);
        a.twist = T.tabs;
        a.L1 = T.L1;
        a.L2 = T.L2;
        a.twist_per_col = T.shared ? 0 : 1;
        a.tw_inv = r.coeffs ? nullptr : ctx->twiddle29(logh, true);
        a.tw_fwd = ctx->twiddle29(logh, false);
    }
    LSP_HIP(launch_ntt(a, ctx->stream));
}

void intt_device(lsp_ctx* ctx, const Fr* in, ColMap map, Fr* out, size_t w, uint32_t logh) {
    const NttLaunch a{.what = LDE_INV, .src = in, .map = map, .scratch = out, .w = w, .logh = logh,
                      .tw_inv = logh ? ctx->twiddle29(logh, true) : nullptr};
    LSP_HIP(launch_ntt(a, ctx->stream));
}

void lde_device(lsp_ctx* ctx, const Fr* d_in, size_t h, size_t w, uint32_t added_bits, const Fr* shifts_host,
                Fr* d_out) {
    lde(ctx, {.src = d_in, .map = ColMap::plain((uint32_t)w), .h = h, .w = w, .added_bits = added_bits,
              .shifts = shifts_host, .out = d_out});
}

// TwoAdicSubgroupDft::coset_dft_batch ([EXT p3-dft]; dft_batch: shift 1): the
// h x w true coefficients at d_coef -> evaluations on shift H_h, stored
// bit-reversed (row j = p(shift w_h^bitrev(j)), Radix2DitParallel's
// Evaluations layout) -- the forward half of the LDE with one block and
// twist s^i instead of s^i / h
void coset_dft_device(lsp_ctx* ctx, const Fr* d_coef, size_t h, size_t w, const Fr& shift, Fr* d_out) {
    LSP_REQUIRE(log2_exact(h) <= 40, LSP_E_SIZE, "transform too large");
    const std::vector<Fr> sh(w, shift);
    lde(ctx, {.src = d_coef, .coeffs = true, .map = ColMap::plain((uint32_t)w), .h = h, .w = w, .shifts = sh.data(),
              .nk = 1, .div_h = false, .out = d_out});
}

// TwoAdicSubgroupDft::coset_idft_batch (idft_batch: shift 1): evaluations on
// shift H_h in natural row order -> the coefficients (natural order,
// canonical): the LDE's inverse half (h c_i), then c_i = X_i (1/h) shift^-i
void coset_idft_device(lsp_ctx* ctx, const Fr* d_evals, size_t h, size_t w, const Fr& shift, Fr* d_out) {
    const uint32_t logh = log2_exact(h);
    LSP_REQUIRE(logh <= 40, LSP_E_SIZE, "transform too large");
    LSP_REQUIRE(!fr_is_zero(fr_to_canonical(shift)), LSP_E_ARG, "coset shift must be nonzero");
    uint32_t L1, L2;
    const size_t per = two_level(logh, L1, L2);
    const Fr base_scale[2] = {host_inv_cached(shift), host_inv_cached(fr_from_u64(h))};
    // (not cached: a caller's shift)
    const Fr* tab = ctx->table("", per, pow_fill(ctx, base_scale, 1, true, L1, L2, true), "idft_tab");
    Fr* X = ctx->fbuf("idft_X", h * w);
    intt_device(ctx, d_evals, ColMap::plain((uint32_t)w), X, w, logh);
    LSP_HIP(launch_scale_coeffs(X, h, (uint32_t)w, tab, L1, d_out, ctx->stream));
}

// Block `blk` (S = N / 2^b rows, S < h) of the bit-reversed N-row LDE, when a
// proof has more ranks than cosets: the evaluations on the sub-coset
// c H_S, c = shift_c w_N^bitrev_b(blk).  The h coefficients of every column
// fold to S (c'_i = sum_t c_(i + t S) c^(t S), SURVEY 8(e) step 6 without a
// transpose), then one size-S coset NTT of the folded columns, which is the
// transform from coefficients with the LDE seen as 2^b blocks of S rows.  The
// fold also divides by f = h / S, so the NTT's 1/S twist scale gives the 1/h
// the coefficients (h * c_i, as the inverse leaves them) need.
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
    lde(ctx, {.src = folded, .coeffs = true, .map = ColMap::plain((uint32_t)w), .h = S, .w = w, .added_bits = b,
              .shifts = shifts_host, .k0 = blk, .nk = 1, .out = d_out});
}

}  // namespace lsp
