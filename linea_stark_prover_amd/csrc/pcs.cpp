// TwoAdicFriPcs over batches of unequal heights:
// commit (coset LDEs under one mixed-height tree, U14), open (opened values,
// one reduced-opening vector per LDE height, a FRI commit phase that rolls each
// shorter vector in where the lengths meet, the queries) and the host
// verifier, with the proof's wire format "LSPPCS01" (DESIGN.md section 9).
// Built on the stage drivers the prover runs (stages.cpp, merkle_mixed.cpp) and
// on its FRI (fri.cpp).  Every FRI round runs on the device: no host tail and
// no host tree top on this path (the commit phase's policy values are 0 here).
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>

#include "comm.hpp"
#include "host.hpp"
#include "prove_internal.hpp"
#include "wire.hpp"

lsp_challenger::lsp_challenger(const lsp_ctx* ctx) : p2(ctx->p2), ch(&p2, ctx->transcript.mont_bits) {}

namespace lsp {

// ------------------------------------------------------------- refusals
void PcsRounds::check(const lsp_ctx* ctx) {
    LSP_REQUIRE(!batches.empty(), LSP_E_ARG, "a PCS opening needs at least one batch");
    const uint32_t lfin = ctx->log_blowup + ctx->log_final_poly_len;
    const Fr GEN = host_generator();
    size_t npoints = 0, nmax = 0;
    for (const auto& B : batches) {
        std::vector<size_t> hs, ws;
        for (const Mat& m : B) {
            hs.push_back(m.N);
            ws.push_back(m.width);
        }
        (void)height_classes(ws.data(), hs.data(), B.size());  // no matrix, widths, heights, classes of more than 8
        for (const Mat& m : B) {
            // the verifier's loop has no round that could take a shorter vector in
            LSP_REQUIRE(log2_exact(m.N) > lfin, LSP_E_SIZE,
                        "an LDE height below 2 * 2^(log_blowup + log_final_poly_len)");
            nmax = std::max(nmax, m.N);
            npoints += m.points.size();
        }
    }
    LSP_REQUIRE(npoints >= 1, LSP_E_ARG, "a PCS opening needs at least one point");
    bool tallest_opened = false;
    for (const auto& B : batches)
        for (const Mat& m : B) {
            tallest_opened = tallest_opened || (m.N == nmax && !m.points.empty());
            if (m.points.empty()) continue;
            const Fr gN = fr_pow_u64(GEN, m.N);  // p3 divides by zero at a point of the matrix's own LDE coset
            for (const Fr& z : m.points)
                LSP_REQUIRE(!fr_eq(fr_pow_u64(z, m.N), gN), LSP_E_ARG, "a point lies on its matrix's LDE coset");
        }
    LSP_REQUIRE(tallest_opened, LSP_E_ARG, "no matrix of the tallest height is opened at a point");
    log_nmax = log2_exact(nmax);
}

// --------------------------------------------------------------- commit
std::unique_ptr<lsp_tree> pcs_commit(lsp_ctx* ctx, const lsp_fr* const* mats, const size_t* heights,
                                     const size_t* widths, const lsp_fr* shifts, size_t n, int mem, Fr* root) {
    const uint32_t lb = ctx->log_blowup;
    const Fr GEN = host_generator();
    std::vector<size_t> N(n);
    for (size_t k = 0; k < n; ++k) {
        LSP_REQUIRE(heights[k] <= (((size_t)1 << 40) >> lb), LSP_E_SIZE, "matrix height beyond 2^40 / blowup");
        N[k] = heights[k] << lb;
    }
    const std::vector<HeightClass> cls = height_classes(widths, N.data(), n);
    std::vector<Fr> lde_shift(n);
    for (size_t k = 0; k < n; ++k) {
        LSP_REQUIRE(log2_exact(N[k]) > lb + ctx->log_final_poly_len, LSP_E_SIZE,
                    "an LDE height below 2 * 2^(log_blowup + log_final_poly_len)");
        LSP_REQUIRE(mats[k], LSP_E_ARG, "null matrix");
        const Fr s = shifts ? to_fr(shifts[k]) : fr_one();
        LSP_REQUIRE(!fr_is_zero(fr_to_canonical(s)), LSP_E_ARG, "domain shift must be nonzero");
        lde_shift[k] = fr_mul(GEN, fr_inv(s));  // evaluations on GEN H_N whatever the domain's shift
    }
    LSP_REQUIRE(ctx->device != LSP_HOST_ONLY, LSP_E_STATE, "host-only context (LSP_HOST_ONLY) has no GPU");
    LSP_HIP(hipSetDevice(ctx->device));
    auto t = new_tree(ctx, cls[0].height, n, N.data(), widths, nullptr, mem);
    for (size_t k = 0; k < n; ++k) {
        const size_t ne = heights[k] * widths[k];
        const Fr* din = reinterpret_cast<const Fr*>(mats[k]);
        if (mem == LSP_MEM_HOST) {
            Fr* d = ctx->fbuf("pcs_in", ne);
            LSP_HIP(hipMemcpyAsync(d, mats[k], ne * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
            din = d;
        }
        const std::vector<Fr> sh(widths[k], lde_shift[k]);
        lde_device(ctx, din, heights[k], widths[k], lb, sh.data(), t->mats[k]);  // straight into the tree's buffer
    }
    *root = commit_mixed_device(ctx, cls, t->mats.data(), widths, t->layers);
    return t;
}

// ----------------------------------------------------------------- open
std::unique_ptr<lsp_pcs_proof> pcs_open(lsp_ctx* ctx, const lsp_tree* const* trees, PcsRounds& R, Challenger& ch) {
    hipStream_t st = ctx->stream;
    const DeferTopUploads defer(ctx);
    SoloComm solo;
    const uint32_t lb = ctx->log_blowup;
    const Fr GEN = host_generator();
    const size_t nb = R.batches.size();
    auto proof = std::make_unique<lsp_pcs_proof>();
    size_t nys = 0, maxw = 0;
    proof->shape.resize(nb);
    for (size_t b = 0; b < nb; ++b)
        for (const PcsRounds::Mat& m : R.batches[b]) {
            proof->shape[b].push_back({(uint32_t)m.width, (uint32_t)m.points.size()});
            nys += m.width * m.points.size();
            maxw = std::max(maxw, m.width);
        }

    // ---- inverse denominators, once per (height, distinct point).  The N
    // denominators are z - x over the coset GEN H_N: their product is
    // z^N - GEN^N, inverted on the host instead of by a Fermat chain on the GPU
    struct Inv {
        uint32_t logN;
        Fr z;
        const Fr* d;
    };
    std::vector<Inv> invs;
    auto inv_of = [&](uint32_t logN, const Fr& z) {
        for (const Inv& e : invs)
            if (e.logN == logN && fr_eq(e.z, z)) return e.d;
        const size_t N = (size_t)1 << logN;
        Fr* d = ctx->fbuf("pcs_inv_" + std::to_string(invs.size()), N);
        const Fr tot = fr_inv(fr_sub(fr_pow_u64(z, N), fr_pow_u64(GEN, N)));
        open_denominators(ctx, z, GEN, logN, 0, N, d, &tot);
        invs.push_back({logN, z, d});
        return (const Fr*)d;
    };

    // ---- opened values: p(z) from the first h rows of each LDE (the coset GEN H_h)
    Fr* sums = ctx->fbuf("pcs_sums", nys);
    {
        size_t o = 0;
        for (size_t b = 0; b < nb; ++b)
            for (size_t k = 0; k < R.batches[b].size(); ++k) {
                const PcsRounds::Mat& m = R.batches[b][k];
                const uint32_t logN = log2_exact(m.N);
                for (const Fr& z : m.points) {
                    barycentric_sums(ctx, trees[b]->mats[k], (uint32_t)m.width, m.N >> lb, inv_of(logN, z), GEN, logN,
                                     0, sums + o);
                    o += m.width;
                }
            }
        Fr* hs = (Fr*)ctx->hbuf("pcs_sums_h", nys * sizeof(Fr));
        LSP_HIP(hipMemcpyAsync(hs, sums, nys * sizeof(Fr), hipMemcpyDeviceToHost, st));
        LSP_HIP(hipStreamSynchronize(st));
        proof->ys.assign(hs, hs + nys);
        o = 0;
        for (size_t b = 0; b < nb; ++b)
            for (const PcsRounds::Mat& m : R.batches[b]) {
                const CosetFactor factor(GEN, m.N >> lb, true);
                for (const Fr& z : m.points) {
                    const Fr f = factor.at(z);
                    for (size_t c = 0; c < m.width; ++c, ++o) proof->ys[o] = fr_mul(proof->ys[o], f);
                }
            }
    }
    if (ctx->transcript.opened_values)  // U7: in the nesting order
        for (const Fr& y : proof->ys) ch.observe(y);
    const Fr alpha = ch.sample();

    // ---- one reduced-opening vector per LDE height; the running power of alpha
    // is per height and runs across the batches in order
    std::map<uint32_t, Fr*> ro;
    {
        const std::vector<Fr> apw = alpha_powers(alpha, maxw + 1);
        std::map<uint32_t, Fr> off;
        struct Launch {
            const Fr *M, *inv;
            Fr* ro;
            size_t N, w;
        };
        std::vector<Launch> todo;
        std::vector<Fr> coef(apw.begin(), apw.begin() + maxw);  // then per launch: off, off * reduced ys
        size_t o = 0;
        for (size_t b = 0; b < nb; ++b)
            for (size_t k = 0; k < R.batches[b].size(); ++k) {
                const PcsRounds::Mat& m = R.batches[b][k];
                if (m.points.empty()) continue;
                const uint32_t logN = log2_exact(m.N);
                if (!ro.count(logN)) {
                    ro[logN] = ctx->fbuf("pcs_ro_" + std::to_string(logN), m.N);
                    off[logN] = fr_one();
                    LSP_HIP(hipMemsetAsync(ro[logN], 0, m.N * sizeof(Fr), st));
                }
                for (const Fr& z : m.points) {
                    coef.push_back(off[logN]);
                    coef.push_back(fr_mul(off[logN], reduce_opened(apw.data(), proof->ys.data() + o, m.width)));
                    todo.push_back({trees[b]->mats[k], inv_of(logN, z), ro[logN], m.N, m.width});
                    off[logN] = fr_mul(off[logN], apw[m.width]);
                    o += m.width;
                }
            }
        Fr* dc = ctx->fbuf("pcs_coef", coef.size());
        ctx->h2d_async("pcs_coef_h", dc, coef.data(), coef.size() * sizeof(Fr));
        F29* consts29 = nullptr;  // alpha powers beyond the LDS: global (every launch's are a prefix of the widest's)
        if (const size_t nsc = reduce_matrix_scratch((uint32_t)maxw, ctx->lds_per_block))
            consts29 = (F29*)ctx->buf("pcs_coef_29", nsc * sizeof(F29));
        for (size_t j = 0; j < todo.size(); ++j) {
            const Launch& l = todo[j];
            LSP_HIP(launch_reduce_matrix(l.M, l.N, (uint32_t)l.w, dc, 1, l.inv, dc + maxw + 2 * j, dc + maxw + 2 * j + 1,
                                         l.ro, ctx->lds_per_block, consts29, st));
        }
    }
    // ---- FRI commit phase (fri.cpp): each shorter vector rolls in where the
    // lengths meet; round 0's input is the tallest vector, the folds go to pcs_fvec
    const size_t nmax = (size_t)1 << R.log_nmax;
    FriCommit fri(
        ctx, solo, ro.at(R.log_nmax), ctx->fbuf("pcs_fvec", nmax), nmax, proof->roots,
        [&](size_t len) -> const Fr* {
            const auto it = ro.find(log2_exact(len));
            return it == ro.end() ? nullptr : it->second;
        },
        0, 0);
    proof->final_poly = fri.final_poly(fri.commit(ch), false, false);
    if (ctx->transcript.final_poly)  // U12
        for (const Fr& c : proof->final_poly) ch.observe(c);
    proof->pow_w = fr_from_u64(grind_device(ctx, ch, ctx->pow_bits));

    // ---- queries: every query's rows, paths and siblings by one gather and one download
    const size_t nq = ctx->num_queries;
    std::vector<size_t> idxs(nq);
    for (size_t& idx : idxs) idx = (size_t)ch.sample_bits(R.log_nmax);
    std::vector<uint64_t> ptrs;
    for (const size_t idx : idxs) {
        for (size_t b = 0; b < nb; ++b) {
            const lsp_tree& t = *trees[b];
            const size_t ib = idx >> (R.log_nmax - log2_exact(t.height));
            for (size_t k = 0; k < t.mats.size(); ++k)
                for (size_t c = 0; c < t.widths[k]; ++c)
                    ptrs.push_back((uint64_t)(uintptr_t)(t.mats[k] + t.row_of(k, ib) * t.widths[k] + c));
            push_path(ptrs, t.layers, t.height, ib);
        }
        fri.push_query(ptrs, idx);
    }
    flush_top_uploads(ctx);  // the gather reads the tree tops
    const Fr* got = gather_to_host(ctx, ptrs);
    const Fr* e = got;
    proof->queries.resize(nq);
    for (lsp_pcs_proof::Query& q : proof->queries) {
        q.rows.resize(nb);
        q.paths.resize(nb);
        for (size_t b = 0; b < nb; ++b) {
            size_t wsum = 0;
            for (const size_t w : trees[b]->widths) wsum += w;
            const uint32_t lg = log2_exact(trees[b]->height);
            q.rows[b].assign(e, e + wsum);
            e += wsum;
            q.paths[b].assign(e, e + lg);
            e += lg;
        }
        q.fpath.resize(fri.rounds.size());
        for (size_t r = 0; r < fri.rounds.size(); ++r) {
            q.sib.push_back(*e++);
            const uint32_t lg = log2_exact(fri.rounds[r].ml);
            q.fpath[r].assign(e, e + lg);
            e += lg;
        }
    }
    return proof;
}

// ---------------------------------------------------------- wire format
// "LSPPCS01" | u32 batches, queries, rounds, final_poly_len
//   | per batch: u32 matrices, per matrix: u32 width, u32 points
//   | opened values [batch][matrix][point][column] | roots[rounds] | final_poly | pow_witness
//   | per query: per batch { row elements, u32 len, path[len] }, per round { sibling, u32 len, path[len] }
// little-endian words, elements as 32-byte little-endian canonical integers
std::vector<uint8_t> pcs_serialize(const lsp_pcs_proof& p) {
    size_t nu32 = 4, nfr = p.ys.size() + p.roots.size() + p.final_poly.size() + 1;
    for (const auto& B : p.shape) nu32 += 1 + 2 * B.size();
    for (const auto& q : p.queries) {
        nu32 += p.shape.size() + p.roots.size();
        nfr += p.roots.size();
        for (size_t b = 0; b < p.shape.size(); ++b) nfr += q.rows[b].size() + q.paths[b].size();
        for (size_t r = 0; r < p.roots.size(); ++r) nfr += q.fpath[r].size();
    }
    std::vector<uint8_t> out(8 + 4 * nu32 + 32 * nfr);
    std::memcpy(out.data(), "LSPPCS01", 8);
    Writer w{out.data() + 8};
    w.u32((uint32_t)p.shape.size());
    w.u32((uint32_t)p.queries.size());
    w.u32((uint32_t)p.roots.size());
    w.u32((uint32_t)p.final_poly.size());
    for (const auto& B : p.shape) {
        w.u32((uint32_t)B.size());
        for (const auto& m : B) {
            w.u32(m.width);
            w.u32(m.npoints);
        }
    }
    w.frs(p.ys);
    w.frs(p.roots);
    w.frs(p.final_poly);
    w.fr(p.pow_w);
    for (const auto& q : p.queries) {
        for (size_t b = 0; b < p.shape.size(); ++b) {
            w.frs(q.rows[b]);
            w.path(q.paths[b]);
        }
        for (size_t r = 0; r < p.roots.size(); ++r) {
            w.fr(q.sib[r]);
            w.path(q.fpath[r]);
        }
    }
    LSP_REQUIRE(w.p == out.data() + out.size(), LSP_E_STATE, "PCS proof serialization size mismatch");
    return out;
}

int pcs_parse(const uint8_t* b, size_t n, lsp_pcs_proof& p) {
    if (n < 8 || std::memcmp(b, "LSPPCS01", 8) != 0) return 1;
    Reader r{b, n};
    r.off = 8;
    const uint32_t nb = r.u32(), nq = r.u32(), nr = r.u32(), nf = r.u32();
    // every batch holds at least its matrix count, every query at least a path length per batch
    if (r.bad || nb < 1 || nb > r.left() / 4) return 1;
    p.shape.assign(nb, {});
    uint64_t nys = 0;
    std::vector<uint64_t> wsum(nb, 0);
    for (uint32_t k = 0; k < nb; ++k) {
        const uint32_t nm = r.u32();
        if (r.bad || nm > r.left() / 8) return 1;
        p.shape[k].resize(nm);
        for (auto& m : p.shape[k]) {
            m.width = r.u32();
            m.npoints = r.u32();
            nys += (uint64_t)m.width * m.npoints;  // (each below 2^64, and held against the bytes left at once)
            wsum[k] += m.width;
            if (nys > r.left() / 32 || wsum[k] > r.left() / 32) return 1;
        }
    }
    if (r.bad) return 1;
    r.frs(p.ys, nys);
    r.frs(p.roots, nr);
    r.frs(p.final_poly, nf);
    p.pow_w = r.fr();
    if (r.bad) return 5;
    if (nq > r.left() / 4) return 12;
    p.queries.assign(nq, {});
    for (auto& q : p.queries) {
        q.rows.resize(nb);
        q.paths.resize(nb);
        for (uint32_t k = 0; k < nb; ++k) {
            r.frs(q.rows[k], wsum[k]);
            r.frs(q.paths[k], r.u32());
        }
        q.sib.resize(nr);
        q.fpath.resize(nr);
        for (uint32_t k = 0; k < nr; ++k) {
            q.sib[k] = r.fr();
            r.frs(q.fpath[k], r.u32());
        }
        if (r.bad) return 12;
    }
    return r.off == r.n ? 0 : 12;
}

// --------------------------------------------------------------- verify
// The checks, in the order a proof meets them: 1 header, 5 body, 12 queries'
// framing or trailing bytes (pcs_parse); 2 the counts against the context and
// the tallest height; 3 the shape against the caller's batches; 6 / 7 the
// proof-of-work witness; per query 9 an input path's length, 8 an input
// opening, 10 a commit-phase opening, 11 the final polynomial.
int pcs_verify_host(const lsp_ctx* ctx, const Fr* commits, PcsRounds& R, const uint8_t* b, size_t n, Challenger& ch) {
    lsp_pcs_proof p;
    if (const int bad = pcs_parse(b, n, p)) return bad;
    const uint32_t lb = ctx->log_blowup, lmax = (uint32_t)R.log_nmax;
    const size_t nb = R.batches.size(), flen = (size_t)1 << ctx->log_final_poly_len;
    const uint32_t nr = lmax - lb - ctx->log_final_poly_len;
    if (p.shape.size() != nb || p.queries.size() != ctx->num_queries || p.roots.size() != nr ||
        p.final_poly.size() != flen)
        return 2;
    for (size_t k = 0; k < nb; ++k) {
        if (p.shape[k].size() != R.batches[k].size()) return 3;
        for (size_t j = 0; j < p.shape[k].size(); ++j)
            if (p.shape[k][j].width != R.batches[k][j].width || p.shape[k][j].npoints != R.batches[k][j].points.size())
                return 3;
    }
    const Fr one = fr_one(), GEN = host_generator();
    if (ctx->transcript.opened_values)
        for (const Fr& y : p.ys) ch.observe(y);
    const Fr alpha = ch.sample();
    std::vector<Fr> betas;
    if (const int bad = fri_replay(ch, ctx, p.roots, p.final_poly, p.pow_w, betas)) return bad;

    struct Batch {
        std::vector<HeightClass> cls;
        std::vector<size_t> widths;
        uint32_t logN;
    };
    std::vector<Batch> batches(nb);
    for (size_t k = 0; k < nb; ++k) {
        std::vector<size_t> hs;
        for (const auto& m : R.batches[k]) {
            hs.push_back(m.N);
            batches[k].widths.push_back(m.width);
        }
        batches[k].cls = height_classes(batches[k].widths.data(), hs.data(), hs.size());
        batches[k].logN = log2_exact(batches[k].cls[0].height);
    }
    for (const lsp_pcs_proof::Query& q : p.queries) {
        const size_t idx = (size_t)ch.sample_bits(lmax);
        // by log2 of the LDE height: the reduced opening, and the running power
        // of alpha, which runs across the batches in order
        std::map<uint32_t, Fr> ro, apow;
        const Fr* ys = p.ys.data();
        for (size_t k = 0; k < nb; ++k) {
            const Batch& B = batches[k];
            const size_t ib = idx >> (lmax - B.logN);
            if (q.paths[k].size() != B.logN) return 9;
            std::vector<lsp_fr> rows, path;
            for (const Fr& x : q.rows[k]) rows.push_back(from_fr(x));
            for (const Fr& x : q.paths[k]) path.push_back(from_fr(x));
            if (!verify_mixed_host(ctx, commits[k], B.cls, B.widths.data(), B.widths.size(), ib, rows.data(), path.data()))
                return 8;
            const Fr* row = q.rows[k].data();
            for (const auto& m : R.batches[k]) {
                const uint32_t logN = log2_exact(m.N);
                if (!m.points.empty()) {
                    const Fr x = fr_mul(GEN, fr_pow_u64(host_two_adic_generator(logN),
                                                        host_bitrev(idx >> (lmax - logN), logN)));
                    Fr& acc = ro.emplace(logN, fr_zero()).first->second;
                    acc = fr_add(acc, reduced_opening_term(row, ys, m.width, m.points.data(), m.points.size(), x, alpha,
                                                           apow.emplace(logN, one).first->second));
                    ys += m.width * m.points.size();
                }
                row += m.width;
            }
        }
        const int bad = fri_check_query(
            ctx->p2, p.roots, betas, p.final_poly, lmax, idx,
            [&](uint32_t l) -> const Fr* {
                const auto it = ro.find(l);
                return it == ro.end() ? nullptr : &it->second;
            },
            [&](uint32_t k) { return q.sib[k]; }, [&](uint32_t k) { return (uint32_t)q.fpath[k].size(); },
            [&](uint32_t k, uint32_t l) { return q.fpath[k][l]; });
        if (bad) return bad;
    }
    return 0;
}

}  // namespace lsp
