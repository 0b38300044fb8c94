// The p3_uni_stark::prove orchestration (bin/src/main.rs:80-86) over the
// device pipelines (coset LDE: lde.cpp; Merkle commit: merkle.cpp; quotient,
// open, FRI: the kernels), on one GPU or as one rank of a sharded proof
// (its exchanges: exchange.cpp).
// The Fiat-Shamir transcript stays on the host (a few dozen hashes); every
// bulk step runs on the device and only roots, opened values and query
// openings cross PCIe.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <optional>

#include "comm.hpp"
#include "host.hpp"
#include "prove_internal.hpp"

namespace lsp {

namespace {
// HIP events around each phase (span names as in the reference's bench.log),
// taken from and returned to the context's event pool: creating and destroying
// ~40 events per proof cost ~60 us of host time at the end of every proof
// Phase events are skipped when the context's phase_timing is off
// (lsp_ctx_set_phase_timing) or LSP_PHASE_EVENTS=0, and for phases outside
// the context's phase_only list when it has one; lsp_last_timings reports the
// phases that were timed
struct PhaseTimer {
    lsp_ctx* ctx;
    bool on;
    std::vector<std::pair<std::string, hipEvent_t>> starts;
    std::vector<std::tuple<std::string, hipEvent_t, hipEvent_t>> done;
    explicit PhaseTimer(lsp_ctx* c) : ctx(c) {
        const char* e = std::getenv("LSP_PHASE_EVENTS");
        on = c->phase_timing && !(e && *e == '0');
    }
    hipEvent_t take() {
        hipEvent_t e;
        if (!ctx->event_pool.empty()) {
            e = ctx->event_pool.back();
            ctx->event_pool.pop_back();
        } else {
            LSP_HIP(hipEventCreate(&e));
        }
        return e;
    }
    bool wanted(const std::string& name) const {
        if (!on) return false;
        if (ctx->phase_only.empty()) return true;
        for (const auto& n : ctx->phase_only)
            if (n == name) return true;
        return false;
    }
    void begin(const std::string& name) {
        if (!wanted(name)) return;
        const hipEvent_t e = take();
        LSP_HIP(hipEventRecord(e, ctx->stream));
        starts.emplace_back(name, e);
    }
    void end(const std::string& name) {
        if (!wanted(name)) return;
        for (size_t i = starts.size(); i-- > 0;) {
            if (starts[i].first == name) {
                const hipEvent_t e = take();
                LSP_HIP(hipEventRecord(e, ctx->stream));
                done.emplace_back(name, starts[i].second, e);
                starts.erase(starts.begin() + i);
                return;
            }
        }
    }
    // hand the phase events over for resolve_timings (no wait here: ~40 us of
    // event queries at the end of every proof otherwise)
    void collect() {
        resolve_timings(ctx);  // a previous proof's, if nobody asked for them
        ctx->timings.clear();
        ctx->pending_timings = std::move(done);
        for (auto& st : starts) ctx->event_pool.push_back(st.second);
        done.clear();
        starts.clear();
    }
};

}  // namespace

void resolve_timings(lsp_ctx* ctx) {
    if (ctx->pending_timings.empty()) return;
    ctx->timings.clear();
    for (auto& t : ctx->pending_timings) {
        LSP_HIP(hipEventSynchronize(std::get<2>(t)));
        float ms = 0;
        LSP_HIP(hipEventElapsedTime(&ms, std::get<1>(t), std::get<2>(t)));
        ctx->timings.emplace_back(std::get<0>(t), (double)ms);
        ctx->event_pool.push_back(std::get<1>(t));
        ctx->event_pool.push_back(std::get<2>(t));
    }
    ctx->pending_timings.clear();
}

// --------------------------------------------------------------- grind
// GrindingChallenger::grind(bits) on the device: the smallest witness w >= 0
// with sample_bits(bits) == 0 after observe(w) (U8).  The sponge over the
// challenger's input buffer is absorbed on the host up to the block that
// will hold w; the device runs the last permutation for 2^22 candidates per
// launch.  The winner is re-checked on the host transcript.
uint64_t grind_device(lsp_ctx* ctx, Challenger& ch, uint32_t bits) {
    if (bits == 0) {
        LSP_REQUIRE(ch.check_witness(0, 0), LSP_E_STATE, "grind(0) must accept w = 0");
        return 0;
    }
    const std::vector<Fr>& in = ch.in;  // observe(w) clears the output buffer and appends w
    Fr s0 = fr_zero(), s1 = fr_zero(), s2 = fr_zero();
    size_t k = 0;
    while (k + 2 <= in.size()) {
        s0 = in[k];
        s1 = in[k + 1];
        ctx->p2.permute(s0, s1, s2);
        k += 2;
    }
    uint32_t wlane;
    Fr pre[3];
    if (k < in.size()) {  // odd prefix: [last, w] form the final block
        pre[0] = in[k];
        pre[1] = s1;
        pre[2] = s2;
        wlane = 1;
    } else {  // even prefix: w alone in lane 0, lane 1 keeps the previous state
        pre[0] = s0;
        pre[1] = s1;
        pre[2] = s2;
        wlane = 0;
    }
    unsigned long long* best = (unsigned long long*)ctx->buf("grind_best", sizeof(unsigned long long));
    const uint64_t batch = 1ull << 22;
    for (uint64_t base = 0;; base += batch) {
        LSP_HIP(hipMemsetAsync(best, 0xff, sizeof(unsigned long long), ctx->stream));
        LSP_HIP(launch_grind(pre, wlane, base, batch, bits, ch.mont_bits, ctx->rc29_dev, ctx->p2.L, best, ctx->stream));
        unsigned long long got = 0;
        LSP_HIP(hipMemcpyAsync(&got, best, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
        LSP_HIP(hipStreamSynchronize(ctx->stream));
        if (got != ~0ull) {
            LSP_REQUIRE(ch.check_witness(bits, got), LSP_E_STATE, "device grind witness rejected by the transcript");
            return got;
        }
        LSP_REQUIRE(base < (1ull << 50), LSP_E_STATE, "grinding did not terminate");
    }
}

// ------------------------------------------------------------- prove
// p3_uni_stark::prove (bin/src/main.rs:80-86) as one rank of a G-rank
// proof; G = 1 is the single-GPU prover.  Rank g owns the
// LDE rows [g S, (g+1) S), S = N / G: whole cosets of the bit-reversed LDE
// (G <= blowup), hence a whole subtree of every input Merkle tree, the
// quotient points whose rows it holds, and a contiguous slice of every FRI
// vector.  Exchanges: subtree roots, the quotient chunks (one allgather),
// the opened values (each computed on one rank's first coset, allgathered), the
// FRI vector once a slice is shorter than FRI_SHARD_MIN, and the query
// openings.  The transcript runs on every rank with identical inputs.
namespace {
// What one rank of the proof owns: computed once by shard_geometry, const afterwards
struct Shard {
    size_t h, w, q;  // trace rows and columns, quotient chunks
    uint32_t log_h, lb, log_q, logN, logQ;
    size_t N, Q;       // rows of the LDE, points of the quotient domain
    uint32_t G, g, b;  // ranks, this rank, log2 G
    uint32_t logS;
    size_t S, row0;  // this rank's LDE rows [row0, row0 + S)
    // G <= 2^lb: rank g owns the whole cosets [k0, k0 + nk).  G > 2^lb (sub): a
    // sub-coset of S < h rows, folded from the coefficients (subcoset_lde)
    bool sub;
    uint32_t nk, k0;
    // split: the inverse NTTs go by columns (exchange_plan).  qsplit: so do the
    // quotient chunks' (sub: a chunk spreads over Gq / q ranks, so the holders
    // broadcast values and every rank inverts the assembled h x q matrix)
    bool split, qsplit;
    // Quotient point i reads LDE rows bitrev_Q(i) and bitrev_Q(i + q): the ranks
    // holding the first Q rows (Gq of them) each own the points
    // i = bitrev(g) mod Gq, which are whole chunks j = i mod q (Gq <= q),
    // cpr of them per rank
    size_t Sq, Gq, cpr;
    uint32_t logGq;
};

Shard shard_geometry(const lsp_ctx* ctx, const Comm& comm, size_t h, size_t w, const Air& air, size_t npub,
                     size_t wp = 0) {
    air.require_fits(w, npub, wp);
    Shard s;
    s.h = h;
    s.w = w;
    s.log_h = log2_exact(h);
    LSP_REQUIRE(h >= 2, LSP_E_SIZE, "trace needs at least 2 rows");
    s.lb = ctx->log_blowup;
    // log2(h) <= log_final_poly_len leaves FRI no commit-phase round, and the
    // verifier's fold chain has no round that could take the reduced opening in
    // (fri_check_query; pcs.cpp refuses the same shape)
    LSP_REQUIRE(s.log_h > ctx->log_final_poly_len, LSP_E_SIZE,
                "an LDE height below 2 * 2^(log_blowup + log_final_poly_len)");
    s.log_q = air.log_quotient_degree(ctx->public_degree);
    LSP_REQUIRE(s.log_q <= s.lb, LSP_E_ARG, "quotient degree exceeds the blowup");
    s.q = (size_t)1 << s.log_q;
    s.logN = s.log_h + s.lb;
    s.logQ = s.log_h + s.log_q;
    s.N = (size_t)1 << s.logN;
    s.Q = (size_t)1 << s.logQ;
    LSP_REQUIRE(s.logN <= 40, LSP_E_SIZE, "trace too large");
    s.G = (uint32_t)comm.size;
    s.g = (uint32_t)comm.rank;
    s.b = log2_exact(s.G);
    LSP_REQUIRE(s.b <= s.lb + 6, LSP_E_ARG, "a proof shards over at most 2^(log_blowup + 6) ranks");
    LSP_REQUIRE(s.b < s.logN, LSP_E_SIZE, "more ranks than LDE rows / 2");
    s.logS = s.logN - s.b;
    s.S = s.N >> s.b;
    s.row0 = (size_t)s.g * s.S;
    s.sub = s.b > s.lb;
    s.nk = s.sub ? 1u : 1u << (s.lb - s.b);
    s.k0 = s.sub ? s.g : s.g * s.nk;
    s.split = s.G > 1 && exchange_plan(comm, h, w, s.q, s.lb).split;
    s.qsplit = s.split && !s.sub;
    s.Sq = std::min(s.S, s.Q);
    s.Gq = s.Q / s.Sq;
    s.cpr = s.q / s.Gq;
    s.logGq = log2_exact(s.Gq);
    return s;
}

// One proof: the state its phases hand on, and the phases in the order
// prove_shard calls them.  The transcript is prove_shard's; only the per-round
// (root, beta) pairs of the FRI commit phase are observed and sampled here.
struct Prover {
    lsp_ctx* const ctx;
    Comm& comm;
    const Fr* const d_trace;
    const Air& air;
    const Fr* const pub;
    const size_t npub;
    const Shard s;
    const hipStream_t st;
    const Fr GEN = host_generator(), one = fr_one();
    const Fr wh, wh_inv;  // the trace domain's generator
    PhaseTimer T;
    std::unique_ptr<lsp_proof> proof;  // released to the caller by finish()
    std::vector<Fr> shifts;
    // One committed matrix as the opening walks it, in the order of proof->mats:
    // this rank's LDE rows, its subtree's layers, the host layers above the rank
    // subtrees (none: the layers hold every level), its width, its points
    struct Committed {
        const Fr* lde = nullptr;
        Fr* layers = nullptr;
        std::vector<std::vector<Fr>> top;
        size_t width = 0;
        uint32_t npoints = 0;
    };
    std::vector<Committed> mats;
    // the trace's LDE, and h * coefficients (split or sub) read through tmap
    Fr* lde = nullptr;
    const Fr* tcoef = nullptr;
    ColMap tmap;
    // the quotient.  G = 1: qv is the h x q chunk matrix.  G > 1: ranks g < Gq
    // evaluate points into their slot of the exchange buffer `stage` (qsplit:
    // into a local buffer, whose inverse NTT goes to the slot)
    QuotientArgs qa;  // alpha set once sampled
    Fr *qv = nullptr, *stage = nullptr, *qloc = nullptr;
    Fr* qlde = nullptr;
    // constraints before alpha: side work issued by the trace tree that the
    // main stream has not waited for yet (side_pending), see early_constraints
    bool early = false, side_pending = false;
    std::function<void(hipEvent_t)> side_fn;
    Fr* inv_z = nullptr;  // 1 / (zeta - x) over this rank's S rows, then 1 / (zeta w_h - x): one buffer, stride S
    // FRI: round 0's input, this rank's slice, at fvec[0, S) with the fold area
    // behind it; the commit phase (fri.cpp)
    Fr* fvec = nullptr;
    std::optional<FriCommit> fri;
    // LSP_TIME_TOPS
    host_clock::time_point t_entry, t_lde_issued, q0, q1, q2, q3;

    Prover(lsp_ctx* c, Comm& cm, const Fr* trace, const Air& a, const Fr* pv, size_t npv, const Shard& geo,
           host_clock::time_point entry)
        : ctx(c), comm(cm), d_trace(trace), air(a), pub(pv), npub(npv), s(geo), st(c->stream),
          wh(host_two_adic_generator(geo.log_h)), wh_inv(host_inv_cached(wh)), T(c), proof(new lsp_proof()),
          t_entry(entry) {
        ctx->spans.clear();
        proof->log_h = s.log_h;
        proof->log_q = s.log_q;
        proof->rehearsal = comm.rehearsal();
        add_matrix(s.w);
        add_matrix(s.q);
        T.begin("prove");
    }
    Prover(const Prover&) = delete;  // side_fn points into this object
    // the main stream never runs ahead of side work it did not wait for
    ~Prover() {
        if (side_pending) (void)hipStreamWaitEvent(ctx->stream, ctx->ev_side, 0);
    }

    // the next committed matrix, in this list and the proof's
    Committed& add_matrix(size_t width) {
        proof->mats.emplace_back(mats.size(), (uint32_t)width);
        mats.push_back({nullptr, nullptr, {}, width, proof->mats.back().npoints});
        return mats.back();
    }

    // the logical operations of p3_uni_stark::prove with their dims, worded as
    // the reference's tracing spans (bench.log:19-64); batched launches
    // are logged per reference call (one quotient chunk, one opened matrix)
    void span(const char* name, size_t rows_w, size_t height, int added_bits) {
        char buf[160];
        if (added_bits >= 0)
            std::snprintf(buf, sizeof buf, "%s dims: %zux%zu | added_bits: %d", name, rows_w, height, added_bits);
        else
            std::snprintf(buf, sizeof buf, "%s dims: %zux%zu", name, rows_w, height);
        ctx->spans.emplace_back(buf);
    }

    // ---- commit to trace data: the LDE, everything of the quotient that does
    // not depend on alpha, and the tree (with the constraint evaluation beside it)
    void commit_trace() {
        T.begin("commit to trace data");
        trace_lde();
        quotient_setup();
        early_constraints();
        Committed& M = mats[MAT_TRACE];
        M.lde = lde;
        M.layers = ctx->fbuf("t_tree", TreeLayout{s.S}.size());
        T.begin("merkle tree");
        proof->mats[MAT_TRACE].root = shard_root(
            ctx, comm, commit_device(ctx, one_mat(lde, (uint32_t)s.w), s.S, M.layers, host_tree_top(ctx), nullptr,
                               early ? &side_fn : nullptr),
            M.top, "trace subtree roots");
        T.end("merkle tree");
        T.end("commit to trace data");
    }

    void trace_lde() {
        const size_t h = s.h, w = s.w;
        lde = ctx->fbuf("t_lde", s.S * w);
        shifts.assign(std::max(w, s.q), GEN);
        T.begin("coset_lde_batch");
        span("coset_lde_batch", w, h, (int)s.lb);
        if (s.split) {
            // rank g inverts the columns bitrev(g) + G k (k < cg; columns past w
            // are zero padding), the ranks allgather the h x cg coefficient
            // blocks, and each transforms its own cosets from them
            const uint32_t cg = (uint32_t)((w + s.G - 1) / s.G);
            Fr* xl = ctx->fbuf("t_coef_local", h * cg);
            Fr* coef = ctx->fbuf("t_coef", h * cg * s.G);
            ColMap m = ColMap::plain((uint32_t)w);
            m.c0 = (uint32_t)host_bitrev(s.g, s.b);
            m.cstep = s.G;
            T.begin("trace inverse NTT");  // this rank's cg columns (tests/test_gpu_calibration.py)
            intt_device(ctx, d_trace, m, xl, cg, s.log_h);
            T.end("trace inverse NTT");
            comm.allgather(ctx, xl, coef, h * cg * sizeof(Fr), "trace coefficients");
            tcoef = coef;
            tmap = ColMap::blocked(s.b, cg);
        } else if (s.sub) {  // every rank inverts every column (LSP_SHARD_SPLIT_INTT=0)
            Fr* coef = ctx->fbuf("t_coef", h * w);
            intt_device(ctx, d_trace, ColMap::plain((uint32_t)w), coef, w, s.log_h);
            tcoef = coef;
            tmap = ColMap::plain((uint32_t)w);
        }
        rank_lde(d_trace, tcoef, tmap, w, lde, "t_sub");
        t_lde_issued = host_clock::now();
        T.end("coset_lde_batch");
    }

    // This rank's rows of one committed matrix's LDE (shifts set by the caller):
    // a sub-coset folded from the coefficients when the proof has more ranks
    // than cosets, else its coset blocks -- from h * coefficients at `coef`
    // through `cmap` where the ranks split the inverse, from the local
    // evaluations otherwise (coef null)
    void rank_lde(const Fr* evals, const Fr* coef, ColMap cmap, size_t w, Fr* out, const char* sub_tag) {
        if (s.sub) return subcoset_lde(ctx, coef, cmap, s.h, w, s.logN, s.b, s.g, shifts.data(), out, sub_tag);
        lsp::lde(ctx, {.src = coef ? coef : evals, .coeffs = coef != nullptr,
                       .map = coef ? cmap : ColMap::plain((uint32_t)w), .h = s.h, .w = w, .added_bits = s.lb,
                       .shifts = shifts.data(), .k0 = s.k0, .nk = s.nk, .out = out});
    }

    // the quotient kernel's buffers and arguments (nothing here depends on alpha)
    void quotient_setup() {
        const size_t h = s.h, w = s.w, q = s.q, S = s.S, Q = s.Q, Sq = s.Sq, Gq = s.Gq;
        const uint32_t G = s.G, g = s.g;
        qv = G == 1 || !s.qsplit ? ctx->fbuf("q_values", Q) : nullptr;
        stage = G == 1 ? nullptr : ctx->fbuf("q_stage", Sq * Gq);
        qloc = G == 1 ? qv
                      : (g < Gq ? (s.qsplit ? ctx->fbuf("q_vals_local", Sq) : stage + (size_t)g * Sq) : nullptr);
        // point i + q (the next trace row) of this rank's points i = i0 + Gq m:
        // on this rank when Gq <= q; else all on the rank with residue
        // (i0 + q) mod Gq, whose LDE rows this rank computes itself
        const Fr* lde_next = nullptr;
        uint64_t row0_next = 0;
        if (s.sub && s.row0 < Q) {
            const uint32_t gn = (uint32_t)host_bitrev((host_bitrev(g, s.logGq) + q) & (Gq - 1), s.logGq);
            if (gn != g) {
                Fr* nl = ctx->fbuf("t_lde_next", S * w);
                subcoset_lde(ctx, tcoef, tmap, h, w, s.logN, s.b, gn, shifts.data(), nl, "t_next");
                lde_next = nl;
                row0_next = (uint64_t)gn * S;
            }
        }
        if (s.row0 >= Q) return;
        quotient_domain(ctx, s.log_h, s.log_q, host_bitrev(g, s.logGq), s.logGq, Sq, air, pub, npub, qa);
        qa.lde = lde;
        qa.w = (uint32_t)w;
        qa.out = qloc;
        qa.row0 = s.row0;
        qa.lde_next = lde_next;
        qa.row0_next = row0_next;
        qa.lde_rows = S;
        qa.lde_next_rows = lde_next ? S : 0;
        if (mats.size() > MAT_PREP && air.has_prog) {  // the same lrow / nrow of the preprocessed LDE
            qa.prep = mats[MAT_PREP].lde;
            qa.wp = (uint32_t)mats[MAT_PREP].width;
        }
    }

    // Constraints before alpha (round 4): every constraint C_j at this rank's
    // points depends on the trace LDE and the public values only; alpha enters
    // as the fold sum_j alpha^(n-1-j) C_j (air/src/lib.rs:116-167 through the
    // folder).  So the constraint values are evaluated on a low-priority side
    // stream once the trace tree's wide levels are done, beside its narrow
    // levels and the host's tree top, where most SIMDs idle; after alpha one
    // short kernel folds them.  For shapes whose evaluation outgrows that window
    // (ncons x points > 2^23: 2^20 rows and up at q = 4, the wide AIRs) the
    // quotient stays one kernel after alpha.  LSP_QUOTIENT_EARLY=0 / 1: never /
    // always (read per proof).
    void early_constraints() {
        const uint32_t ncons = (uint32_t)air.stats(ctx->public_degree).second;
        if (s.row0 < s.Q && !s.sub && ncons > 0) {
            const char* e = std::getenv("LSP_QUOTIENT_EARLY");
            early = e && *e ? *e != '0' : (uint64_t)ncons * s.Sq <= (1ull << 23);
        }
        if (!early) return;
        hipStream_t s2 = ctx->side();
        qa.cons = (uint32_t*)ctx->buf("q_cons", (size_t)ncons * 9 * s.Sq * sizeof(uint32_t));
        qa.ncons = ncons;
        side_fn = [this, s2](hipEvent_t ev) {  // commit_device calls it once the tree's wide levels are issued
            LSP_HIP(hipStreamWaitEvent(s2, ev, 0));
            LSP_HIP(launch_quotient(qa, s2));
            LSP_HIP(hipEventRecord(ctx->ev_side, s2));
            side_pending = true;
        };
    }

    // ---- quotient: the constraint fold by alpha, divided by Z_H
    void quotient(const Fr& alpha) {
        const size_t Sq = s.Sq;
        T.begin("compute quotient polynomial");
        if (s.row0 < s.Q) {
            qa.alpha = alpha;
            if (early) {
                LSP_REQUIRE(side_pending, LSP_E_STATE, "the constraint evaluation was not issued");
                LSP_HIP(hipStreamWaitEvent(st, ctx->ev_side, 0));
                side_pending = false;
                LSP_HIP(launch_quotient_fold(qa, st));
            } else {
                LSP_HIP(launch_quotient(qa, st));
            }
        }
        if (s.G > 1) {
            // rank r < Gq holds chunks j = bitrev(r) + Gq c as an h x cpr matrix: one
            // broadcast per holder (only the Gq holders send: Gq/G of an allgather's bytes).
            // split: the holder sends its chunks' coefficients (its own inverse
            // NTT), and no rank inverts the whole h x q matrix
            if (s.qsplit && s.g < s.Gq)
                intt_device(ctx, qloc, ColMap::plain((uint32_t)s.cpr), stage + (size_t)s.g * Sq, s.cpr, s.log_h);
            for (uint32_t r = 0; r < s.Gq; ++r)
                comm.bcast(ctx, stage + (size_t)r * Sq, Sq * sizeof(Fr), (int)r,
                           s.qsplit ? "quotient chunk coefficients" : "quotient values");
            if (!s.qsplit) LSP_HIP(launch_assemble_chunks(stage, s.logGq, Sq, qv, st));
        }
        T.end("compute quotient polynomial");
    }

    // ---- commit to quotient chunks: qv is the h x q matrix of chunks
    void commit_quotient() {
        const size_t h = s.h, q = s.q;
        T.begin("commit to quotient poly chunks");
        const Fr gQ = host_two_adic_generator(s.logQ), gQinv = host_inv_cached(gQ);
        {
            Fr x = one;
            for (size_t j = 0; j < q; ++j) {
                shifts[j] = x;  // GEN / (GEN * w_Q^j)
                x = fr_mul(x, gQinv);
            }
        }
        qlde = ctx->fbuf("q_lde", s.S * q);
        T.begin("coset_lde_batch (quotient)");
        for (size_t j = 0; j < q; ++j) span("coset_lde_batch", 1, h, (int)s.lb);  // one launch, q independent columns
        const Fr* qcoef = nullptr;
        ColMap qmap = ColMap::plain((uint32_t)q);
        if (s.qsplit) {  // the chunk coefficients straight from the exchange buffer (column j in slot bitrev(j mod Gq))
            qcoef = stage;
            qmap = ColMap::blocked(s.logGq, (uint32_t)s.cpr);
        } else if (s.sub) {
            Fr* qc = ctx->fbuf("q_coef", h * q);
            intt_device(ctx, qv, qmap, qc, q, s.log_h);
            qcoef = qc;
        }
        rank_lde(qv, qcoef, qmap, q, qlde, "q_sub");
        T.end("coset_lde_batch (quotient)");
        Committed& M = mats[MAT_QUOTIENT];
        M.lde = qlde;
        M.layers = ctx->fbuf("q_tree", TreeLayout{s.S}.size());
        proof->mats[MAT_QUOTIENT].root = shard_root(
            ctx, comm, commit_device(ctx, one_mat(qlde, (uint32_t)q), s.S, M.layers, host_tree_top(ctx)), M.top,
            "quotient subtree roots");
        T.end("commit to quotient poly chunks");
    }

    // ---- open: the trace at zeta and zeta w_h, the chunks at zeta
    void open_values(const Fr& zeta) {
        const size_t h = s.h, S = s.S, row0 = s.row0;
        const uint32_t G = s.G, g = s.g, logN = s.logN;
        const Fr zeta_next = fr_mul(zeta, wh);
        T.begin("open");
        inverse_denominators(zeta, zeta_next);
        T.begin("compute opened values with Lagrange interpolation");
        // Barycentric sums over one coset c H_h of the LDE domain: p(z) =
        // (z^h - c^h) / (h c^h) * sum_i p(x_i) x_i / (z - x_i).  Any coset gives
        // the same (unique) value, so with whole cosets per rank the three jobs
        // (trace at zeta, trace at zeta*w_h, the chunks at zeta) go to the ranks
        // that evaluated no quotient points (g >= Gq), each over its first coset,
        // instead of all to rank 0; an allgather of the values replaces rank 0's
        // broadcast.  sub: the low coset's h / S ranks add partial sums.
        // The jobs are the (matrix, point) pairs in the list's order.
        struct Job {
            const Committed* m;
            uint32_t point;
            size_t off;  // of its sums among all the jobs'
            bool here;
        };
        std::vector<Job> jobs;
        size_t nsum = 0, maxw = 0;
        const uint32_t nfree = G > s.Gq ? (uint32_t)(G - s.Gq) : 0u;
        bool any_here = false;
        for (const Committed& m : mats) {
            maxw = std::max(maxw, m.width);
            for (uint32_t p = 0; p < m.npoints; ++p, nsum += m.width) {
                // sub: ranks 0 .. h/S - 1 hold the low coset's partial sums of every job
                const uint32_t j = (uint32_t)jobs.size();
                const bool here = s.sub ? row0 < h : g == (nfree ? G - 1 - j % nfree : G - 1 - j % G);
                jobs.push_back({&m, p, nsum, here});
                any_here = any_here || here;
            }
        }
        Fr* sums = ctx->fbuf("o_sums", nsum);
        const size_t nlow = std::min(S, h);  // this rank's rows of one coset
        if (any_here) {
            ctx->fbuf("o_partial", ((nlow + 1023) / 1024) * maxw);  // the drivers' scratch, sized once for the widest job
            for (const Job& j : jobs)
                if (j.here)
                    barycentric_sums(ctx, j.m->lde, (uint32_t)j.m->width, nlow, inv_z + j.point * S, GEN, logN, row0,
                                     sums + j.off);
        }
        Fr* hs = (Fr*)ctx->hbuf("o_sums_h", nsum * sizeof(Fr));  // pinned
        if (any_here) {
            LSP_HIP(hipMemcpyAsync(hs, sums, nsum * sizeof(Fr), hipMemcpyDeviceToHost, st));
            LSP_HIP(hipStreamSynchronize(st));
        }
        // the coset of this rank's first rows: c = GEN w_N^bitrev(row0) (sub: the low coset, GEN)
        const Fr cpos = s.sub ? GEN : fr_mul(GEN, fr_pow_u64(host_two_adic_generator(logN), host_bitrev(row0, logN)));
        const CosetFactor factor(cpos, h, true);
        const Fr z[2] = {zeta, zeta_next};
        for (const Job& j : jobs) {
            const Fr f = factor.at(z[j.point]);
            for (size_t k = 0; k < j.m->width; ++k) hs[j.off + k] = j.here ? fr_mul(hs[j.off + k], f) : fr_zero();
        }
        if (G > 1) {  // every value from its job's rank(s): the sum over ranks
            const std::vector<Fr> all = comm.allgather_fr(ctx, hs, nsum, "opened values");
            for (size_t k = 0; k < nsum; ++k) {
                Fr acc = fr_zero();
                for (uint32_t r = 0; r < G; ++r) acc = fr_add(acc, all[(size_t)r * nsum + k]);
                hs[k] = acc;
            }
        }
        const Fr* y = hs;  // a matrix's jobs lie back to back: its opened values per point
        for (OpenedMat& m : proof->mats) {
            m.ys.assign(y, y + (size_t)m.npoints * m.width);
            y += m.ys.size();
        }
        T.end("compute opened values with Lagrange interpolation");
    }

    // inv_z, inv_zn over this rank's rows
    void inverse_denominators(const Fr& zeta, const Fr& zeta_next) {
        const size_t S = s.S, row0 = s.row0;
        const uint32_t logN = s.logN;
        T.begin("compute_inverse_denominators");
        inv_z = ctx->fbuf("o_invz", 2 * S);
        Fr* const inv_zn = inv_z + S;
        // this rank's rows are the coset c H_S (c = GEN w_N^bitrev(row0)), so the
        // product of its denominators is prod (zeta - c w) = zeta^S - c^S: its
        // inverse on the host replaces the batch inverse's Fermat chain on the GPU
        const Fr cS = fr_pow_u64(fr_mul(GEN, fr_pow_u64(host_two_adic_generator(logN), host_bitrev(row0, logN))), S);
        const Fr den_prod = fr_sub(fr_pow_u64(zeta, S), cS);
        LSP_REQUIRE(!fr_is_zero(den_prod), LSP_E_STATE, "zeta lies in the LDE domain");
        const Fr den_prod_inv = fr_inv(den_prod);
        open_denominators(ctx, zeta, GEN, logN, row0, S, inv_z, &den_prod_inv);
        if (s.sub) {
            // x w_h^-1 leaves a sub-coset (w_h is not in H_S): the zeta_next
            // denominators are inverted on their own
            const Fr dpn = fr_sub(fr_pow_u64(zeta_next, S), cS);
            LSP_REQUIRE(!fr_is_zero(dpn), LSP_E_STATE, "zeta * w_h lies in the LDE domain");
            const Fr dpn_inv = fr_inv(dpn);
            open_denominators(ctx, zeta_next, GEN, logN, row0, S, inv_zn, &dpn_inv);
        } else {
            LSP_HIP(launch_shift_inverse(inv_z, inv_zn, wh_inv, logN, 1ull << s.lb, row0, S, st));
        }
        T.end("compute_inverse_denominators");
    }

    // the first FRI vector: every opened matrix reduced by powers of alpha_fri
    void reduce_rows(const Fr& alpha_fri) {
        const size_t w = s.w, q = s.q;
        T.begin("reduce rows");
        // the (matrix, point) order of TwoAdicFriPcs::open that the reduction
        // below folds in (k_reduce_rows): trace at zeta, trace at zeta*w_h,
        // then quotient chunk j at zeta
        span("reduce matrix quotient", w, s.N, -1);
        span("reduce matrix quotient", w, s.N, -1);
        for (size_t j = 0; j < q; ++j) span("reduce matrix quotient", 1, s.N, -1);
        const OpenedMat &tm = proof->mats[MAT_TRACE], &qm = proof->mats[MAT_QUOTIENT];
        std::vector<Fr> apw = alpha_powers(alpha_fri, 2 * w + q);
        const Fr ry_z = reduce_opened(apw.data(), tm.at(0), w);
        const Fr ry_zn = reduce_opened(apw.data(), tm.at(1), w);
        Fr* dapw = ctx->fbuf("o_apw", apw.size() + q);
        const size_t napw = apw.size();
        apw.insert(apw.end(), qm.ys.begin(), qm.ys.end());
        ctx->h2d_async("o_apw_h", dapw, apw.data(), apw.size() * sizeof(Fr));
        fvec = ctx->fbuf("f_vec", 2 * s.S);
        ReduceArgs ra;
        ra.lde = lde;
        ra.w = (uint32_t)w;
        ra.qlde = qlde;
        ra.q = (uint32_t)q;
        ra.inv_z = inv_z;
        ra.inv_zn = inv_z + s.S;
        ra.apw = dapw;
        ra.ry_z = ry_z;
        ra.ry_zn = ry_zn;
        ra.ryq = dapw + napw;
        ra.out = fvec;
        ra.n = s.S;
        ra.lds_max = ctx->lds_per_block;
        if (const size_t nsc = reduce_rows_scratch(ra.w, ra.q, ra.lds_max))  // constants beyond the LDS: global
            ra.consts29 = (F29*)ctx->buf("o_rr_consts", nsc * sizeof(F29));
        LSP_HIP(launch_reduce_rows(ra, st));
        // the matrices after the fused pair (the preprocessed one), each at zeta
        // and zeta*w_h, continue the running power: accumulated into fvec
        Fr off = fr_pow_u64(alpha_fri, 2 * w + q);
        for (size_t m = MAT_QUOTIENT + 1; m < mats.size(); ++m) {
            span("reduce matrix preprocessed at zeta", mats[m].width, s.N, -1);
            span("reduce matrix preprocessed at zeta*w", mats[m].width, s.N, -1);
            reduce_matrix(ctx, mats[m].lde, s.S, mats[m].width, inv_z, proof->mats[m].ys.data(), mats[m].npoints,
                          alpha_fri, off, fvec, "o_apw_prep");
        }
        T.end("reduce rows");
    }

    // ---- FRI commit phase (fri.cpp): no roll-in; the host takes the tree tops
    // and the last rounds.  Returns the final vector.
    std::vector<Fr> fri_commit(Challenger& ch) {
        T.begin("FRI prover");
        T.begin("commit phase");
        fri.emplace(ctx, comm, fvec, fvec + s.S, s.N, proof->roots, [](size_t) { return (const Fr*)nullptr; },
                    host_tree_top(ctx), ctx->fri_host_tail);
        std::vector<Fr> fin = fri->commit(ch);
        T.end("commit phase");
        return fin;
    }

    // ---- query phase: the owner of a query's row (rank idx / S) gathers the
    // openings below the rank subtrees in one kernel; the layers above come
    // from the host top trees every rank holds.
    void begin_query_phase() {
        flush_top_uploads(ctx);  // the gather reads the tree tops
        T.begin("query phase");
        q0 = host_clock::now();
    }

    void query_phase(const std::vector<size_t>& idxs) {
        q1 = host_clock::now();
        const uint32_t nq = (uint32_t)idxs.size();
        // elements per query below the rank subtrees: per matrix its row and path
        // (one rank: logS = logN, the whole path), then the FRI openings
        size_t E = fri->query_elems();
        for (const Committed& m : mats) E += m.width + s.logS;
        std::vector<uint64_t> ptrs;
        std::vector<uint32_t> mine;
        query_pointers(idxs, ptrs, mine);
        LSP_REQUIRE(ptrs.size() == mine.size() * E, LSP_E_STATE, "query opening layout mismatch");
        // one rank: every query is this rank's, in order, so the gathered openings
        // are already the all-ranks layout and the records read them in place
        // (two host copies of ~E * nq elements fewer between proofs)
        const bool in_place = s.G == 1;
        std::vector<Fr> slots(in_place ? 0 : (size_t)nq * E, fr_zero());
        const Fr* opened = nullptr;  // the openings of every query, (owner rank, query)-major
        if (!ptrs.empty()) {
            const Fr* got = gather_to_host(ctx, ptrs);
            if (in_place)
                opened = got;
            else
                for (size_t k = 0; k < mine.size(); ++k)
                    std::copy(got + k * E, got + (k + 1) * E, slots.begin() + (size_t)mine[k] * E);
        }
        q2 = host_clock::now();
        std::vector<Fr> all;
        if (!in_place) {
            all = comm.allgather_fr(ctx, slots.data(), slots.size(), "query openings");
            opened = all.data();
        }
        LSP_REQUIRE(opened || nq == 0, LSP_E_STATE, "query openings missing");
        query_records(idxs, opened, E);
        q3 = host_clock::now();
        T.end("query phase");
    }

    // the addresses of this rank's queries' openings (E per query), and which queries they are
    void query_pointers(const std::vector<size_t>& idxs, std::vector<uint64_t>& ptrs, std::vector<uint32_t>& mine) {
        for (uint32_t qi = 0; qi < idxs.size(); ++qi) {
            const size_t idx = idxs[qi];
            if ((idx >> s.logS) != s.g) continue;
            mine.push_back(qi);
            const size_t li = idx - s.row0;
            for (const Committed& m : mats) {
                for (size_t c = 0; c < m.width; ++c) ptrs.push_back((uint64_t)(uintptr_t)(m.lde + li * m.width + c));
                push_path(ptrs, m.layers, s.S, li);
            }
            fri->push_query(ptrs, idx);
        }
    }

    // each query's record is independent: assembled (and serialized)
    // on the host pool -- ~0.1 + 0.2 ms of one thread's time at 2^19
    void query_records(const std::vector<size_t>& idxs, const Fr* opened, size_t E) {
        const size_t nq = idxs.size();
        const uint32_t logS = s.logS, nr = (uint32_t)fri->rounds.size();
        auto top_path = [&](const std::vector<std::vector<Fr>>& top, size_t sub, std::vector<Fr>& out) {
            for (uint32_t i = 0; i + 1 < top.size(); ++i) out.push_back(top[i][(sub >> i) ^ 1]);
        };
        // records of a freed proof keep their vectors' capacity (proof_release)
        proof->queries = recycled_queries();
        proof->queries.resize(nq);
        const char* qp = std::getenv("LSP_QUERY_POOL");  // =0: one thread, wire bytes on demand (A/B)
        const bool qpool = !(qp && *qp == '0');
        HostPool serial_pool(0);
        (qpool ? ctx->host_pool() : serial_pool).parallel_for(nq, [&](size_t qi) {
            const size_t idx = idxs[qi], o = idx >> logS;
            const Fr* e = opened + (o * nq + qi) * E;
            lsp_query& qq = proof->queries[qi];
            qq.sib.clear();
            qq.sib.reserve(nr);
            qq.fpath.resize(nr);
            qq.open.resize(mats.size());
            for (size_t m = 0; m < mats.size(); ++m) {
                lsp_query::Opening& op = qq.open[m];
                op.row.assign(e, e + mats[m].width);
                e += mats[m].width;
                op.path.assign(e, e + logS);
                e += logS;
                top_path(mats[m].top, o, op.path);  // (no host layers: the tree's own hold every level)
            }
            for (uint32_t r = 0; r < nr; ++r) {
                const FriRound& R = fri->rounds[r];
                qq.sib.push_back(*e++);
                const uint32_t lg = log2_exact(R.ml);
                std::vector<Fr>& pth = qq.fpath[r];
                pth.assign(e, e + lg);
                e += lg;
                if (R.sharded) top_path(R.top, o, pth);
            }
        });
        // the wire bytes now, in parallel (lsp_proof_serialize returns the cached copy)
        if (qpool) {
            std::vector<uint8_t> buf = recycled_wire();
            proof->wire = serialize(*proof, &ctx->host_pool(), &buf);
        }
    }

    lsp_proof* finish() {
        T.end("FRI prover");
        T.end("open");
        T.end("prove");
        T.collect();
        if (time_tops())
            std::fprintf(stderr,
                         "[query] samples %.1f us, gather+sync %.1f us, assemble %.1f us, collect %.1f us; "
                         "entry -> LDE issued %.1f us\n",
                         us(q0, q1), us(q1, q2), us(q2, q3), us(q3, host_clock::now()), us(t_entry, t_lde_issued));
        return proof.release();
    }
};
}  // namespace

lsp_proof* prove_shard(lsp_ctx* ctx, Comm& comm, const Fr* d_trace, size_t h, size_t w, const Air& air,
                       const Fr* pub, size_t npub, const lsp_tree* prep) {
    const auto t_entry = host_clock::now();
    const ActiveProof active;
    const DeferTopUploads defer(ctx);
    comm.begin_log(ctx);
    const size_t wp = prep && !prep->widths.empty() ? prep->widths[0] : 0;
    const Shard geo = shard_geometry(ctx, comm, h, w, air, npub, wp);
    Prover P(ctx, comm, d_trace, air, pub, npub, geo, t_entry);
    if (prep) {
        LSP_REQUIRE(geo.G == 1, LSP_E_ARG, "a preprocessed matrix is proved on one rank only");
        // the tree's own context: its layers went up on this stream (a commit's host-made
        // top is uploaded asynchronously) and this call holds the mutex that guards them
        LSP_REQUIRE(prep->ctx == ctx, LSP_E_ARG, "the preprocessed tree belongs to another context");
        LSP_REQUIRE(prep->height == geo.N && prep->mats.size() == 1 && wp >= 1, LSP_E_ARG,
                    "the preprocessed tree is not over one matrix of height h << log_blowup");
        LSP_REQUIRE(reduce_matrix_scratch((uint32_t)wp, ctx->lds_per_block) == 0, LSP_E_ARG,
                    "the preprocessed matrix is wider than the reduce kernel's LDS holds");
        // the third committed matrix: the tree's LDE and layers, all on the
        // device; its root is the verifier's own input
        auto& M = P.add_matrix(wp);
        M.lde = prep->mats[0];
        M.layers = prep->layers;
        P.proof->mats[MAT_PREP].root = d2h_fr(ctx, prep->layers + TreeLayout{geo.N}.root());
    }

    P.commit_trace();
    // U7: the instance, then the quotient challenge (TranscriptCfg switches)
    const TranscriptCfg& TC = ctx->transcript;
    Challenger ch(&ctx->p2, TC.mont_bits);
    if (TC.log_degree) ch.observe(fr_from_u64(geo.log_h));
    ch.observe(P.proof->mats[MAT_TRACE].root);
    if (prep) ch.observe(P.proof->mats[MAT_PREP].root);  // U13
    if (TC.public_values)
        for (size_t i = 0; i < npub; ++i) ch.observe(pub[i]);
    const Fr alpha = ch.sample();

    P.quotient(alpha);
    P.commit_quotient();
    ch.observe(P.proof->mats[MAT_QUOTIENT].root);
    const Fr zeta = ch.sample();

    // alpha_fri is sampled once the opened values exist: U7 may observe them
    // first; the default samples it right after zeta, and nothing touches the
    // transcript in between
    P.open_values(zeta);
    if (TC.opened_values)  // U7: every opened value, in (matrix, point) order, before alpha_fri
        for (const OpenedMat& m : P.proof->mats)
            for (const Fr& v : m.ys) ch.observe(v);
    const Fr alpha_fri = ch.sample();

    P.reduce_rows(alpha_fri);
    const std::vector<Fr> fin = P.fri_commit(ch);  // per round: observe(root), beta = sample()
    P.proof->final_poly = P.fri->final_poly(fin, true, comm.rehearsal());
    if (TC.final_poly)  // U12
        for (const Fr& c : P.proof->final_poly) ch.observe(c);
    P.T.begin("grind for proof-of-work witness");
    P.proof->pow_w = fr_from_u64(grind_device(ctx, ch, ctx->pow_bits));
    P.T.end("grind for proof-of-work witness");

    P.begin_query_phase();
    std::vector<size_t> idxs(ctx->num_queries);
    for (size_t& idx : idxs) idx = (size_t)ch.sample_bits(geo.logN);
    P.query_phase(idxs);
    return P.finish();
}

lsp_proof* prove_device(lsp_ctx* ctx, const Fr* d_trace, size_t h, size_t w, const Air& air, const Fr* pub,
                        size_t npub, const lsp_tree* prep) {
    SoloComm solo;
    return prove_shard(ctx, solo, d_trace, h, w, air, pub, npub, prep);
}

}  // namespace lsp
