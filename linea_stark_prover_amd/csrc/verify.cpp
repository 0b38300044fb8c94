// Host CPU verifier: p3_uni_stark::verify (bin/src/main.rs:88-96) with
// TwoAdicFriPcs::verify and the FRI query checks ([EXT p3-fri]).  The
// reference verifies in ~1 s on the CPU (bench.log:69); it stays on the host.
#include <cstring>

#include "prove_internal.hpp"
#include "wire.hpp"

namespace lsp {

namespace {
bool mk_verify(const P2Host& p2, const Fr& root, size_t index, const Fr* leaf, size_t nleaf, Reader& r,
               uint32_t expect) {
    const uint32_t pl = r.u32();
    if (pl != expect) return false;
    const Fr got = merkle_path_root(p2, p2.hash(leaf, nleaf), index, pl, [&](uint32_t) { return r.fr(); }, no_injection);
    return !r.bad && fr_eq(got, root);
}
// the check a committed matrix's query opening fails (host.hpp MAT_*)
constexpr int OPENING_CHECK[] = {8, 9, 14};
}  // namespace

// prep_commit (optional) with prep_width: the verifier's own data about the
// AIR's preprocessed matrix (p3's VerifierData), never proof fields.  Such a
// proof is "LSPPRF03": the list of committed matrices (host.hpp) is one longer,
// and everything below walks that list -- the header's width, the opened values
// (observed in its order), each query's openings and the FRI input, where the
// running alpha_fri power goes through every matrix at each of its points.  The
// preprocessed root is observed after the trace root (U13).  Each format is
// rejected where the other is expected.
int verify_host(const lsp_ctx* ctx, const Air& air, const Fr* pub, size_t npub, const uint8_t* b, size_t n,
                const Fr* prep_commit, uint32_t prep_width) {
    if (npub < 2) return 1;
    if (n < 8 || std::memcmp(b, prep_commit ? "LSPPRF03" : "LSPPRF02", 8) != 0) return 2;
    Reader r{b, n};
    r.off = 8;
    const uint32_t log_h = r.u32(), log_q = r.u32(), w = r.u32(), nq = r.u32(), nr = r.u32(), nf = r.u32();
    const uint32_t wp = prep_commit ? r.u32() : 0;
    if (wp != prep_width || wp > (1u << 20) || air.prep_width > wp || (prep_commit && wp == 0)) return 3;
    if (r.bad || log_q != air.log_quotient_degree(ctx->public_degree) || nq != ctx->num_queries || log_h > 40 ||
        log_h < 1 || w <= air.max_col || w > (1u << 20) || air.max_pub >= (int64_t)npub)
        return 3;
    const uint32_t lb = ctx->log_blowup, logN = log_h + lb;
    // a proof without a commit-phase round is never valid: the fold chain of a
    // query starts from zero and takes the reduced opening in at its first round
    if (log_h <= ctx->log_final_poly_len) return 4;
    if (nr != logN - lb - ctx->log_final_poly_len || nf != (1u << ctx->log_final_poly_len)) return 4;
    const size_t q = (size_t)1 << log_q, h = (size_t)1 << log_h;
    const size_t flen = (size_t)1 << ctx->log_final_poly_len;
    const uint32_t widths[] = {w, (uint32_t)q, wp};
    std::vector<OpenedMat> mats;
    size_t nys = 0, maxw = 0;
    for (size_t m = 0; m < (prep_commit ? 3u : 2u); ++m) {
        mats.emplace_back(m, widths[m]);
        mats[m].root = mats[m].root_on_wire ? r.fr() : *prep_commit;
        nys += (size_t)mats[m].npoints * widths[m];
        maxw = std::max<size_t>(maxw, widths[m]);
    }
    if (r.n - r.off < nys * 32) return 5;  // (before any allocation by a claimed width)
    std::vector<Fr> roots(nr), betas, fp(flen);
    for (OpenedMat& m : mats) {
        m.ys.resize((size_t)m.npoints * m.width);
        for (auto& x : m.ys) x = r.fr();
    }
    for (auto& x : roots) x = r.fr();
    for (auto& x : fp) x = r.fr();
    const Fr pw = r.fr();
    if (r.bad) return 5;
    const Fr one = fr_one(), GEN = host_generator();
    const TranscriptCfg& TC = ctx->transcript;  // U7 / U8 / U12, as the prover
    Challenger ch(&ctx->p2, TC.mont_bits);
    if (TC.log_degree) ch.observe(fr_from_u64(log_h));
    ch.observe(mats[MAT_TRACE].root);
    for (const OpenedMat& m : mats)
        if (!m.root_on_wire) ch.observe(m.root);  // U13: the verifier's own commitments
    if (TC.public_values)
        for (size_t i = 0; i < npub; ++i) ch.observe(pub[i]);
    const Fr alpha = ch.sample();
    ch.observe(mats[MAT_QUOTIENT].root);
    const Fr zeta = ch.sample();
    const Fr wh = host_two_adic_generator(log_h), wh_inv = fr_inv(wh);
    const Fr points[2] = {zeta, fr_mul(zeta, wh)};
    if (TC.opened_values)
        for (const OpenedMat& m : mats)
            for (const Fr& v : m.ys) ch.observe(v);
    const Fr alpha_fri = ch.sample();
    if (const int bad = fri_replay(ch, ctx, roots, fp, pw, betas)) return bad;
    const Fr gN = host_two_adic_generator(logN);
    std::vector<Fr> row(maxw);
    for (uint32_t qi = 0; qi < nq; ++qi) {
        const size_t idx = (size_t)ch.sample_bits(logN);
        const Fr x = fr_mul(GEN, fr_pow_u64(gN, host_bitrev(idx, logN)));
        Fr ro = fr_zero(), apow = one;
        for (size_t m = 0; m < mats.size(); ++m) {
            const OpenedMat& M = mats[m];
            for (uint32_t c = 0; c < M.width; ++c) row[c] = r.fr();
            if (!mk_verify(ctx->p2, M.root, idx, row.data(), M.width, r, logN)) return OPENING_CHECK[m];
            ro = fr_add(ro, reduced_opening_term(row.data(), M.ys.data(), M.width, points, M.npoints, x, alpha_fri, apow));
        }
        // the commit-phase openings, read from the stream as the chain asks for them
        const int bad = fri_check_query(
            ctx->p2, roots, betas, fp, logN, idx, [&](uint32_t l) { return l == logN ? &ro : nullptr; },
            [&](uint32_t) { return r.fr(); }, [&](uint32_t) { return r.u32(); },
            [&](uint32_t, uint32_t) { return r.fr(); });
        if (bad || r.bad) return bad ? bad : 10;
    }
    if (r.bad || r.off != r.n) return 12;
    // out-of-domain identity: folded_constraints(zeta) / Z_H(zeta) == sum zps_i * chunk_i
    const Fr gQ = host_two_adic_generator(log_h + log_q);
    std::vector<Fr> sh(q);
    sh[0] = GEN;
    for (size_t j = 1; j < q; ++j) sh[j] = fr_mul(sh[j - 1], gQ);
    auto zp = [&](const Fr& s, const Fr& xx) { return fr_sub(fr_pow_u64(fr_mul(xx, fr_inv(s)), h), one); };
    const Fr* qc = mats[MAT_QUOTIENT].at(0);
    Fr quotient = fr_zero();
    for (size_t i = 0; i < q; ++i) {
        Fr prod = one;
        for (size_t j = 0; j < q; ++j)
            if (j != i) prod = fr_mul(prod, fr_mul(zp(sh[j], zeta), fr_inv(zp(sh[j], sh[i]))));
        quotient = fr_add(quotient, fr_mul(prod, qc[i]));
    }
    const Fr zh = fr_sub(fr_pow_u64(zeta, h), one);
    const Fr first = fr_mul(zh, fr_inv(fr_sub(zeta, one)));
    const Fr last = fr_mul(zh, fr_inv(fr_sub(zeta, wh_inv)));
    const Fr trans = fr_sub(zeta, wh_inv);
    Fr acc = fr_zero();
    const OpenedMat &T = mats[MAT_TRACE], &P = mats.back();  // (P: read only when it is the preprocessed matrix)
    air.eval_fold(T.at(0), T.at(1), pub, first, last, trans, alpha, acc, prep_commit ? P.at(0) : nullptr,
                  prep_commit ? P.at(1) : nullptr);
    if (!fr_eq(fr_mul(acc, fr_inv(zh)), quotient)) return 13;
    return 0;
}

}  // namespace lsp
