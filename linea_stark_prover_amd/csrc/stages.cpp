// One driver per proof stage: the setup and the launches that the Prover's
// phases (prove.cpp) and the C stage API (capi.cpp) share, so the stage tests
// run the code a proof runs.  Tables come from pow_table, small host arrays go
// up through h2d_async (host temporaries may die at return), inverses of
// domain constants through host_inv_cached -- never of a caller's point or
// shift, which would grow that process-wide map without bound -- and all
// work is on ctx->stream.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "host.hpp"
#include "prove_internal.hpp"

namespace lsp {

// ------------------------------------------------------------ quotient
void quotient_domain(lsp_ctx* ctx, uint32_t log_h, uint32_t log_q, uint64_t i0, uint32_t log_step, size_t n,
                     const Air& air, const Fr* pub, size_t npub, QuotientArgs& qa) {
    const uint32_t logQ = log_h + log_q;
    const size_t h = (size_t)1 << log_h, q = (size_t)1 << log_q;
    if (n == 0) n = ((size_t)1 << logQ) >> log_step;
    LSP_REQUIRE(n == ((size_t)1 << logQ) >> log_step, LSP_E_STATE, "quotient points are not one residue class");
    hipStream_t st = ctx->stream;
    const Fr GEN = host_generator(), one = fr_one();
    const Fr wh_inv = host_inv_cached(host_two_adic_generator(log_h));
    uint32_t L1Q;
    const Fr* tabQ = pow_table(ctx, host_two_adic_generator(logQ), logQ, L1Q);
    // 1/((x-1)(x-w_h^-1)) depends on the domain only: cached per shape in the
    // context (API callers with ever new shapes: a scratch buffer, lsp_ctx::table)
    char key[64];
    std::snprintf(key, sizeof key, "qsel_%u_%u_%llu_%u", log_h, logQ, (unsigned long long)i0, log_step);
    const Fr* inv_den = ctx->table(
        key, n,
        [&](Fr* inv) {
            Fr* den = ctx->fbuf("q_den", n);
            LSP_HIP(launch_selector_denoms(tabQ, L1Q, GEN, wh_inv, n, den, st, i0, log_step));
            LSP_HIP(launch_batch_inverse(den, inv, n, st, ctx->bi_scratch(n)));
        },
        "q_invden");
    std::vector<Fr> zh(2 * q);  // Z_H on the q cosets of H_h in the quotient domain, then their inverses
    {
        const Fr gh = fr_pow_u64(GEN, h), gq = host_two_adic_generator(log_q);
        Fr x = one;
        for (size_t k = 0; k < q; ++k) {
            zh[k] = fr_sub(fr_mul(gh, x), one);
            zh[q + k] = host_inv_cached(zh[k]);
            x = fr_mul(x, gq);
        }
    }
    Fr* dzh = ctx->fbuf("q_zh", 2 * q);
    ctx->h2d_async("q_zh_h", dzh, zh.data(), 2 * q * sizeof(Fr));
    // (air.dev is air.raw unless the descriptor holds a program)
    int32_t* dair = (int32_t*)ctx->buf("air", air.dev.size() * sizeof(int32_t));
    ctx->h2d_async("air_h", dair, air.dev.data(), air.dev.size() * sizeof(int32_t));
    qa.logQ = logQ;
    qa.log_q = log_q;
    qa.air = dair;
    qa.air_len = (uint32_t)air.dev.size();
    qa.pub_alpha = pub[0];
    qa.pub_delta = pub[1];
    if (air.has_prog) {  // programs read the public values from a table
        Fr* dpub = ctx->fbuf("q_pub", npub);
        ctx->h2d_async("q_pub_h", dpub, pub, npub * sizeof(Fr));
        qa.pub = dpub;
        qa.npub = (uint32_t)npub;
        qa.prog = 1;
        qa.prog_slots = air.prog_slots;
    }
    qa.gen = GEN;
    qa.wh_inv = wh_inv;
    qa.tabQ = tabQ;
    qa.L1 = L1Q;
    qa.zh = dzh;
    qa.inv_zh = dzh + q;
    qa.inv_den = inv_den;
    qa.i0 = i0;
    qa.log_step = log_step;
    qa.n = n;
}

// ---------------------------------------------------------------- open
void open_denominators(lsp_ctx* ctx, const Fr& z, const Fr& shift, uint32_t logN, uint64_t row0, size_t n, Fr* out,
                       const Fr* inv_total) {
    uint32_t L1N;
    const Fr* tabN = pow_table(ctx, host_two_adic_generator(logN), logN, L1N);
    Fr* den = ctx->fbuf("o_den", n);
    LSP_HIP(launch_open_denoms(z, shift, tabN, L1N, logN, n, den, ctx->stream, row0));
    LSP_HIP(launch_batch_inverse(den, out, n, ctx->stream, ctx->bi_scratch(n), inv_total));
}

void barycentric_sums(lsp_ctx* ctx, const Fr* M, uint32_t w, size_t n, const Fr* inv_den, const Fr& shift,
                      uint32_t logN, uint64_t row0, Fr* sums) {
    uint32_t L1N;
    const Fr* tabN = pow_table(ctx, host_two_adic_generator(logN), logN, L1N);
    Fr* partial = ctx->fbuf("o_partial", ((n + 1023) / 1024) * w);
    uint32_t nb = 0;
    LSP_HIP(launch_interp_partial(M, w, n, inv_den, shift, tabN, L1N, logN, partial, &nb, ctx->stream, row0));
    LSP_HIP(launch_sum_partials(partial, nb, w, sums, ctx->stream));
}

CosetFactor::CosetFactor(const Fr& c, size_t h_, bool domain_constant) : h(h_), ch(fr_pow_u64(c, h_)) {
    const Fr d = fr_mul(ch, fr_from_u64(h));
    inv_hch = domain_constant ? host_inv_cached(d) : fr_inv(d);
}

// ----------------------------------------------------------------- FRI
FoldSpec fold_spec(lsp_ctx* ctx, uint32_t logm, uint64_t i0, const Fr& beta) {
    FoldSpec f{};
    f.half = host_inv_cached(fr_from_u64(2));
    f.half_beta = fr_mul(beta, f.half);
    f.tab = pow_table(ctx, host_inv_cached(host_two_adic_generator(logm + 1)), logm, f.L1);
    f.logm = logm;
    f.i0 = i0;
    return f;
}

void fri_fold(lsp_ctx* ctx, const FoldSpec& f, size_t m) {
    LSP_HIP(launch_fri_fold(f, m, ctx->stream));
}

// -------------------------------------------------------------- reduce
std::vector<Fr> alpha_powers(const Fr& alpha, size_t n) {
    std::vector<Fr> apw(n);
    Fr pw = fr_one();
    for (size_t k = 0; k < n; ++k) {
        apw[k] = pw;
        pw = fr_mul(pw, alpha);
    }
    return apw;
}

Fr reduce_opened(const Fr* apw, const Fr* ys, size_t w) {
    Fr ry = fr_zero();
    for (size_t c = 0; c < w; ++c) ry = fr_add(ry, fr_mul(apw[c], ys[c]));
    return ry;
}

void reduce_matrix(lsp_ctx* ctx, const Fr* M, size_t n, size_t w, const Fr* inv, const Fr* ys, size_t npts,
                   const Fr& alpha, Fr& off, Fr* ro, const std::string& tag) {
    // for the kernel: alpha^c (c < w), then per point the running power, then
    // per point that power times the opened values reduced by the alpha^c
    std::vector<Fr> coef = alpha_powers(alpha, w + 1);
    const Fr aw = coef[w];  // alpha^w: the running power advances by the matrix width
    coef.resize(w + 2 * npts);
    for (size_t p = 0; p < npts; ++p) {
        coef[w + p] = off;
        coef[w + npts + p] = fr_mul(off, reduce_opened(coef.data(), ys + p * w, w));
        off = fr_mul(off, aw);
    }
    Fr* dc = ctx->fbuf(tag, coef.size());
    ctx->h2d_async(tag + "_h", dc, coef.data(), coef.size() * sizeof(Fr));
    F29* consts29 = nullptr;  // alpha powers beyond the LDS: global
    if (const size_t nsc = reduce_matrix_scratch((uint32_t)w, ctx->lds_per_block))
        consts29 = (F29*)ctx->buf(tag + "_29", nsc * sizeof(F29));
    LSP_HIP(launch_reduce_matrix(M, n, (uint32_t)w, dc, (uint32_t)npts, inv, dc + w, dc + w + npts, ro,
                                 ctx->lds_per_block, consts29, ctx->stream));
}

}  // namespace lsp
