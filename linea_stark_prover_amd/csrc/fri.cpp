// FRI, once: the commit phase the prover (prove.cpp) and
// the PCS (pcs.cpp) both run -- FriCommit --, the query phase's shared pieces
// (push_path, gather_to_host), and the verifier's transcript replay and
// per-query fold chain (fri_replay, fri_check_query) that verify.cpp and
// pcs.cpp's verifier both call.  The two callers differ in policy values
// (host tree top, host tail), in the roll-in hook and in where round 0's input
// lives; nothing else.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "comm.hpp"
#include "host.hpp"
#include "prove_internal.hpp"

namespace lsp {

// ------------------------------------------------------------ commit phase
FriCommit::FriCommit(lsp_ctx* c, Comm& cm, const Fr* input, Fr* fold_area, size_t n, std::vector<Fr>& roots_out,
                     AddOfLen add, size_t tree_top, size_t tail)
    : ctx(c), comm(cm), b(log2_exact((size_t)cm.size)), g((uint32_t)cm.rank),
      final_len((size_t)1 << (c->log_blowup + c->log_final_poly_len)),
      host_tree_top(env_size("LSP_HOST_TREE_TOP", tree_top)), host_tail(env_size("LSP_FRI_HOST_TAIL", tail)),
      // (tests lower the shortest slice worth a collective per round to shard every round)
      fri_shard_min(std::max<size_t>(1, env_size("LSP_FRI_SHARD_MIN", (size_t)1 << 12))), add_of_len(std::move(add)),
      roots(roots_out), cur(input), area(fold_area), len(n), sharded(cm.size > 1) {
    ftree = ctx->fbuf("f_tree", 2 * (n >> b) + 2 * (size_t)cm.size * fri_shard_min);
}

std::vector<Fr> FriCommit::commit(Challenger& ch) {
    hipStream_t st = ctx->stream;
    const Fr* hfin = nullptr;  // the final vector, when the host ran the last rounds
    while (len > final_len) {
        if (sharded && (len >> b) < 2 * fri_shard_min) {
            flush_fold();  // the gathered vector must exist
            replicate();
        }
        if (!sharded && host_tail_fits()) {
            hfin = fri_host_tail(ch);
            break;
        }
        fri_device_round(ch);
    }
    flush_fold();
    if (sharded) replicate();
    std::vector<Fr> fin(len);
    if (hfin)
        std::copy(hfin, hfin + len, fin.begin());
    else {
        Fr* hf = (Fr*)ctx->hbuf("f_final_h", len * sizeof(Fr));
        LSP_HIP(hipMemcpyAsync(hf, cur, len * sizeof(Fr), hipMemcpyDeviceToHost, st));
        LSP_HIP(hipStreamSynchronize(st));
        std::copy(hf, hf + len, fin.begin());
    }
    return fin;
}

// the host folds without a roll-in: its rounds start only below the last one
bool FriCommit::host_tail_fits() const {
    if (len / 2 > host_tail) return false;
    for (size_t l = len / 2; l >= final_len; l /= 2)
        if (add_of_len(l)) return false;
    return true;
}

void FriCommit::replicate() {  // gather the short vector to every rank
    const size_t loc = len >> b;
    Fr* rep = ctx->fbuf("f_rep", 2 * len);
    comm.allgather(ctx, cur, rep, loc * sizeof(Fr), "FRI vector");
    cur = rep;
    area = rep + len;
    ao = 0;
    sharded = false;
}

void FriCommit::flush_fold() {  // the fold no later leaf kernel will run
    if (!pending) return;
    fri_fold(ctx, pend, pend_m);
    pending = false;
}

// one round on the device: the tree (with the previous round's fold and
// roll-in fused into its leaves), then this round's fold left pending
void FriCommit::fri_device_round(Challenger& ch) {
    const size_t m = len / 2, ml = sharded ? (m >> b) : m;
    FriRound R;
    R.vec = cur;
    R.tree = ftree + to;
    R.ml = ml;
    R.sharded = sharded;
    const Fr lroot = commit_device(ctx, one_mat(cur, 2), ml, ftree + to, host_tree_top, pending ? &pend : nullptr);
    pending = false;
    const Fr root = sharded ? shard_root(ctx, comm, lroot, R.top, "FRI subtree roots") : lroot;
    roots.push_back(root);
    ch.observe(root);
    const Fr beta = ch.sample();
    const uint64_t i0 = sharded ? (uint64_t)g * ml : 0;
    pend = fold_spec(ctx, log2_exact(m), i0, beta);
    pend.v = cur;
    pend.vout = area + ao;
    if (const Fr* add = add_of_len(m)) pend.add = add + i0;
    pend_m = ml;
    pending = true;
    rounds.push_back(std::move(R));
    cur = area + ao;
    ao += ml;
    to += TreeLayout{ml}.size();
    len = m;
}

// The last rounds wholly on the host: their trees are a few thousand
// permutations in a chain of short levels (~58 us each on the GPU, a few
// us on the host pool).  One download of the vector; per round the host
// hashes the tree, samples beta and folds; the layers and folded vectors
// go back asynchronously for the query openings, which gather on the device.
// Returns the final vector (in the pinned "fri_tail" buffer).
const Fr* FriCommit::fri_host_tail(Challenger& ch) {
    hipStream_t st = ctx->stream;
    flush_fold();
    const auto th0 = host_clock::now();
    size_t hn = final_len, ht = 0;
    for (size_t l = len; l > final_len; l /= 2) {
        hn += l;
        ht += l - 1;
    }
    Fr* hv = (Fr*)ctx->hbuf("fri_tail", (hn + ht) * sizeof(Fr));
    Fr* htr = hv + hn;
    LSP_HIP(hipMemcpyAsync(hv, cur, len * sizeof(Fr), hipMemcpyDeviceToHost, st));
    LSP_HIP(hipStreamSynchronize(st));
    const auto th1 = host_clock::now();
    const size_t rounds_gpu = rounds.size();
    size_t hvo = 0, hto = 0;
    const size_t to0 = to, ao0 = ao, len0 = len;
    while (len > final_len) {
        const size_t end = fri_host_round(ch, hv + hvo, htr + hto);
        hvo += len;
        hto += end;
        to += end;
        len /= 2;
    }
    // every round's layers and folded vector back to the device (for the
    // query gather): both are contiguous, so two copies instead of two per round
    LSP_HIP(hipMemcpyAsync(ftree + to0, htr, (to - to0) * sizeof(Fr), hipMemcpyHostToDevice, st));
    LSP_HIP(hipMemcpyAsync(area + ao0, hv + len0, (hvo + len - len0) * sizeof(Fr), hipMemcpyHostToDevice, st));
    if (time_tops())
        std::fprintf(stderr, "[fri tail] %zu rounds on the host: %.1f us (download %.1f us)\n",
                     rounds.size() - rounds_gpu, us(th0, host_clock::now()), us(th0, th1));
    return hv + hvo;
}

// one host round over v[0, len): its tree into lay (returns the layers'
// length), the root and beta, the folded vector to v + len
size_t FriCommit::fri_host_round(Challenger& ch, Fr* v, Fr* lay) {
    const size_t m = len / 2;
    const uint32_t logm = log2_exact(m);
    const Fr half = host_inv_cached(fr_from_u64(2));
    const auto tr0 = host_clock::now();
    // leaves (a 2-element leaf's hash_iter is compress, A4/A5) and levels in one pass
    auto tr1 = tr0;
    const size_t end = host_levels(ctx, lay, m, &tr1, v);
    const auto tr2 = host_clock::now();
    FriRound R;
    R.vec = cur;
    R.tree = ftree + to;
    R.ml = m;
    R.sharded = false;
    const Fr root = lay[end - 1];
    roots.push_back(root);
    ch.observe(root);
    const Fr hb = fr_mul(ch.sample(), half);
    std::vector<Fr>& tw = ctx->fold_tw[logm];  // g^-bitrev(i), g = w_{2m}
    if (tw.size() != m) {
        const Fr ginv = host_inv_cached(host_two_adic_generator(logm + 1));
        std::vector<Fr> pw(m);
        pw[0] = fr_one();
        for (size_t j = 1; j < m; ++j) pw[j] = fr_mul(pw[j - 1], ginv);
        tw.resize(m);
        for (size_t i = 0; i < m; ++i) tw[i] = pw[host_bitrev(i, logm)];
    }
    Fr* out = v + len;
    // half (v0 + v1) + hb g^-bitrev(i) (v0 - v1), in the 64-bit lazy
    // form; short vectors on this thread (a pool round trip costs more)
    const hp64::F hh = hp64::from(half), hbb = hp64::from(hb);
    auto fold_blk = [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
            const hp64::F a = hp64::from(v[2 * i]), b2 = hp64::from(v[2 * i + 1]);
            const hp64::F p = hp64::mul(hbb, hp64::from(tw[i]));
            out[i] = hp64::to_canonical(hp64::add(hp64::mul(hh, hp64::add(a, b2)), hp64::mul(p, hp64::sub(a, b2))));
        }
    };
    if (m <= 256)
        fold_blk(0, m);
    else
        ctx->host_pool().parallel_for((m + 63) / 64,
                                      [&](size_t blk) { fold_blk(64 * blk, std::min(m, 64 * blk + 64)); });
    if (time_tops())
        std::fprintf(stderr, "[fri tail round] m %5zu  leaves %6.1f  levels %6.1f  challenge+fold+copies %6.1f us\n", m,
                     us(tr0, tr1), us(tr1, tr2), us(tr2, host_clock::now()));
    rounds.push_back(std::move(R));
    cur = area + ao;
    ao += m;
    return end;
}

// final poly: bit-reverse, IDFT (naive: at most 2^(log_blowup + log_final_poly_len) values), truncate
std::vector<Fr> FriCommit::final_poly(const std::vector<Fr>& fin, bool span, bool rehearsal) const {
    const size_t n = fin.size();
    if (span) ctx->spans.emplace_back("divide_by_height dims: 1x" + std::to_string(n));
    const uint32_t lgl = log2_exact(n);
    std::vector<Fr> br(n), out;
    for (size_t i = 0; i < n; ++i) br[i] = fin[host_bitrev(i, lgl)];
    const Fr winv = host_inv_cached(host_two_adic_generator(lgl));
    const Fr linv = host_inv_cached(fr_from_u64(n));
    const size_t flen = (size_t)1 << ctx->log_final_poly_len;
    for (size_t k = 0; k < n; ++k) {
        Fr acc = fr_zero();
        const Fr wk = fr_pow_u64(winv, k);
        Fr p = fr_one();
        for (size_t j = 0; j < n; ++j) {
            acc = fr_add(acc, fr_mul(br[j], p));
            p = fr_mul(p, wk);
        }
        acc = fr_mul(acc, linv);
        if (k < flen)
            out.push_back(acc);
        else  // (a rehearsal rank's fabricated peer data folds to no polynomial: not checked)
            LSP_REQUIRE(fr_is_zero(acc) || rehearsal, LSP_E_STATE, "FRI final polynomial degree too high");
    }
    return out;
}

// ------------------------------------------------------------- query phase
size_t FriCommit::query_elems() const {
    size_t e = 0;
    for (const FriRound& R : rounds) e += 1 + log2_exact(R.ml);
    return e;
}

void FriCommit::push_query(std::vector<uint64_t>& ptrs, size_t idx) const {
    for (size_t r = 0; r < rounds.size(); ++r) {
        const FriRound& R = rounds[r];
        const size_t ii = idx >> r;                                // global index in round r's vector
        const size_t base = R.sharded ? (size_t)g * 2 * R.ml : 0;  // global index of R.vec[0]
        ptrs.push_back((uint64_t)(uintptr_t)(R.vec + ((ii ^ 1) - base)));
        push_path(ptrs, R.tree, R.ml, (ii >> 1) - base / 2);
    }
}

void push_path(std::vector<uint64_t>& ptrs, const Fr* layers, size_t leaves, size_t leaf) {
    const TreeLayout lay{leaves};
    for (uint32_t l = 0, n = lay.levels(); l < n; ++l)
        ptrs.push_back((uint64_t)(uintptr_t)(layers + lay.sibling(l, leaf)));
}

const Fr* gather_to_host(lsp_ctx* ctx, const std::vector<uint64_t>& ptrs) {
    hipStream_t st = ctx->stream;
    // the gather reads its pointer list from pinned host memory and writes the
    // openings into coherent pinned memory: no copy either side of the kernel
    // (LSP_GATHER_ZEROCOPY=0: upload, gather to HBM, download; read per call)
    const char* zc = std::getenv("LSP_GATHER_ZEROCOPY");
    Fr* got;
    if (!(zc && *zc == '0')) {
        uint64_t* hp = (uint64_t*)ctx->hbuf("g_ptrs_zc", ptrs.size() * sizeof(uint64_t));
        std::memcpy(hp, ptrs.data(), ptrs.size() * sizeof(uint64_t));
        got = (Fr*)ctx->hbuf("g_out_zc", ptrs.size() * sizeof(Fr), hipHostMallocCoherent);
        LSP_HIP(launch_gather(hp, got, ptrs.size(), st));
    } else {
        uint64_t* dptrs = (uint64_t*)ctx->buf("g_ptrs", ptrs.size() * sizeof(uint64_t));
        Fr* dgot = ctx->fbuf("g_out", ptrs.size());
        ctx->h2d_async("g_ptrs_h", dptrs, ptrs.data(), ptrs.size() * sizeof(uint64_t));
        LSP_HIP(launch_gather(dptrs, dgot, ptrs.size(), st));
        got = (Fr*)ctx->hbuf("g_out_h", ptrs.size() * sizeof(Fr));  // pinned: no staging copy
        LSP_HIP(hipMemcpyAsync(got, dgot, ptrs.size() * sizeof(Fr), hipMemcpyDeviceToHost, st));
    }
    LSP_HIP(hipStreamSynchronize(st));
    return got;
}

// ---------------------------------------------------------------- verifier
// TwoAdicFriGenericConfig::fold_row
Fr fold_row(size_t index, uint32_t log_height, const Fr& beta, const Fr& e0, const Fr& e1) {
    const Fr s0 = fr_pow_u64(host_two_adic_generator(log_height + 1), host_bitrev(index, log_height));
    return fr_add(e0, fr_mul(fr_mul(fr_sub(beta, s0), fr_sub(e1, e0)), fr_inv(fr_sub(fr_neg(s0), s0))));
}

int fri_replay(Challenger& ch, const lsp_ctx* ctx, const std::vector<Fr>& roots, const std::vector<Fr>& final_poly,
               const Fr& pow_w, std::vector<Fr>& betas) {
    betas.resize(roots.size());
    for (size_t k = 0; k < roots.size(); ++k) {
        ch.observe(roots[k]);
        betas[k] = ch.sample();
    }
    if (ctx->transcript.final_poly)  // U12
        for (const Fr& c : final_poly) ch.observe(c);
    const Fr pwc = fr_to_canonical(pow_w);
    for (int i = 2; i < 8; ++i)
        if (pwc.v[i]) return 6;
    if (!ch.check_witness(ctx->pow_bits, (uint64_t)pwc.v[0] | ((uint64_t)pwc.v[1] << 32))) return 7;
    return 0;
}

int fri_check_query(const P2Host& p2, const std::vector<Fr>& roots, const std::vector<Fr>& betas,
                    const std::vector<Fr>& final_poly, uint32_t lmax, size_t index,
                    const std::function<const Fr*(uint32_t)>& ro_of_log_height,
                    const std::function<Fr(uint32_t)>& sib, const std::function<uint32_t(uint32_t)>& path_len,
                    const std::function<Fr(uint32_t, uint32_t)>& path) {
    const uint32_t nr = (uint32_t)roots.size();
    Fr folded = fr_zero();
    for (uint32_t k = 0; k < nr; ++k) {
        const uint32_t log_folded = lmax - 1 - k;
        if (const Fr* ro = ro_of_log_height(log_folded + 1)) folded = fr_add(folded, *ro);  // the roll-in: plain addition
        Fr ev[2];
        ev[(index ^ 1) & 1] = sib(k);
        ev[index & 1] = folded;
        if (path_len(k) != log_folded) return 10;
        const Fr got = merkle_path_root(
            p2, p2.hash(ev, 2), index >> 1, log_folded, [&](uint32_t l) { return path(k, l); }, no_injection);
        if (!fr_eq(got, roots[k])) return 10;
        index >>= 1;
        folded = fold_row(index, log_folded, betas[k], ev[0], ev[1]);
    }
    // final polynomial at x^(2^nr) (constant when log_final_poly_len = 0)
    const Fr xf = fr_pow_u64(host_two_adic_generator(lmax - nr), host_bitrev(index, lmax - nr));
    Fr ev = fr_zero();
    for (size_t k = final_poly.size(); k-- > 0;) ev = fr_add(fr_mul(ev, xf), final_poly[k]);
    return fr_eq(ev, folded) ? 0 : 11;
}

}  // namespace lsp
