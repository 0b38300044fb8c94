#pragma once
#include <chrono>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "host.hpp"

namespace lsp {
struct Comm;
// LSP_TIME_TOPS=1 (merkle.cpp): host-side timing of the tree tops, the FRI
// host tail and the query phase, printed to stderr
bool time_tops();
using host_clock = std::chrono::steady_clock;
inline double us(host_clock::time_point a, host_clock::time_point b) {
    return std::chrono::duration<double, std::micro>(b - a).count();
}
// the unsigned value of environment variable `name`, or dflt when it is not set
inline size_t env_size(const char* name, size_t dflt) {
    const char* e = std::getenv(name);
    return e ? (size_t)std::strtoull(e, nullptr, 10) : dflt;
}
// ---- lde.cpp
// two-level power table of `base` covering exponents < 2^bits, cached in the context
const Fr* pow_table(lsp_ctx* ctx, const Fr& base, uint32_t bits, uint32_t& L1);
Fr d2h_fr(lsp_ctx* ctx, const Fr* d);  // one element from the device (synchronises the stream)
// One device transform to coset evaluations: the coset blocks [k0, k0 + nk)
// of the bit-reversed LDE of an h x w matrix by 2^added_bits.  Block k = rows
// k*h .. (k+1)*h - 1 of the full LDE, the evaluations on shift_c *
// w_N^bitrev(k) * H_h; `out` receives the nk blocks.
struct LdeRequest {
    const Fr* src = nullptr;  // the values on H_h, rows in natural order, or (coeffs) h * coefficients, natural
    bool coeffs = false;      // order: the forward half alone, for ranks that split the inverse
    ColMap map;               // where the w columns sit in src
    size_t h = 0, w = 0;
    uint32_t added_bits = 0;
    const Fr* shifts = nullptr;  // one per column (host)
    uint32_t k0 = 0, nk = 0;     // nk = 0: all 2^added_bits blocks
    bool div_h = true;           // false: src holds true coefficients (coset_dft)
    Fr* out = nullptr;
};
void lde(lsp_ctx* ctx, const LdeRequest& r);
// the inverse half: out (h x w) <- h * coefficients, natural order, of the w columns `map` picks in `in`
void intt_device(lsp_ctx* ctx, const Fr* in, ColMap map, Fr* out, size_t w, uint32_t logh);
// block `blk` (N / 2^b < h rows) of the N-row LDE, folded from the coefficients; buffers named after `tag`
void subcoset_lde(lsp_ctx* ctx, const Fr* coef, ColMap map, size_t h, size_t w, uint32_t logN, uint32_t b,
                  uint32_t blk, const Fr* shifts_host, Fr* d_out, const std::string& tag);
// ---- stages.cpp: one driver per proof stage, shared by the Prover's phases and the C stage API
// The quotient domain of a 2^log_h-row trace with 2^log_q chunks, for the
// points i = i0 + (m << log_step), m < n (one residue class; n = 0: all of it):
// fills every field of `qa` that depends neither on alpha nor on where the LDE
// rows live (logQ, log_q, air, air_len, pub_*, gen, wh_inv, tabQ, L1, zh,
// inv_zh, inv_den, i0, log_step, n).  Owns the context's "qsel_*" cache of
// inverted selector denominators.
void quotient_domain(lsp_ctx* ctx, uint32_t log_h, uint32_t log_q, uint64_t i0, uint32_t log_step, size_t n,
                     const Air& air, const Fr* pub, size_t npub, QuotientArgs& qa);
// out[i] = 1 / (z - shift w_N^bitrev(row0 + i)), i < n.  inv_total (optional):
// 1 / (the product of the n denominators) where the caller knows it in closed form
void open_denominators(lsp_ctx* ctx, const Fr& z, const Fr& shift, uint32_t logN, uint64_t row0, size_t n, Fr* out,
                       const Fr* inv_total = nullptr);
// Barycentric interpolation over a coset c H_h: p(z) = factor(z) * sum_i p(x_i) x_i / (z - x_i).
// sums[c] = sum_{i < n} M[i][c] x_i inv_den[i], x_i = shift w_N^bitrev(row0 + i), for the n x w matrix M
void barycentric_sums(lsp_ctx* ctx, const Fr* M, uint32_t w, size_t n, const Fr* inv_den, const Fr& shift,
                      uint32_t logN, uint64_t row0, Fr* sums);
// factor(z) = (z^h - c^h) / (h c^h); domain_constant: c is one (its inverse goes through host_inv_cached)
struct CosetFactor {
    size_t h;
    Fr ch, inv_hch;
    CosetFactor(const Fr& c, size_t h, bool domain_constant);
    Fr at(const Fr& z) const { return fr_mul(fr_sub(fr_pow_u64(z, h), ch), inv_hch); }
};
// the FRI fold by beta of a vector of global folded length 2^logm, for the
// pairs from global pair index i0 on (v, vout and the roll-in add are the
// caller's to set); fri_fold launches it for m pairs
FoldSpec fold_spec(lsp_ctx* ctx, uint32_t logm, uint64_t i0, const Fr& beta);
void fri_fold(lsp_ctx* ctx, const FoldSpec& f, size_t m);
// alpha^k, k < n, and a row of opened values reduced by them: sum_c apw[c] ys[c], c < w
std::vector<Fr> alpha_powers(const Fr& alpha, size_t n);
Fr reduce_opened(const Fr* apw, const Fr* ys, size_t w);
// One matrix's terms of a reduced opening, added to ro (device, n): the n x w
// device matrix M at npts >= 1 points, inv[p n + i] its inverse denominators
// (device), ys[p w + c] its opened values (host).  off: as apow below; buffers named after `tag`
void reduce_matrix(lsp_ctx* ctx, const Fr* M, size_t n, size_t w, const Fr* inv, const Fr* ys, size_t npts,
                   const Fr& alpha, Fr& off, Fr* ro, const std::string& tag);
// ---- Merkle trees
// Where a tree's digests live in its one array, leaves first: level l (the
// leaves are level 0) holds leaves >> l nodes from offset(l) on.
struct TreeLayout {
    size_t leaves;  // a power of two
    uint32_t levels() const {  // above the leaves = the length of a path
        uint32_t n = 0;
        while (((size_t)1 << n) < leaves) ++n;
        return n;
    }
    size_t len(uint32_t level) const { return leaves >> level; }
    size_t offset(uint32_t level) const { return 2 * leaves - (2 * leaves >> level); }
    size_t offset_of_len(size_t n) const { return 2 * (leaves - n); }  // of the level with n nodes
    size_t root() const { return 2 * leaves - 2; }
    size_t size() const { return 2 * leaves - 1; }
    // the path element of `level` in the opening at leaf `index`
    size_t sibling(uint32_t level, size_t index) const { return offset(level) + ((index >> level) ^ 1); }
};
// The root a path leads to from the digest `cur` of leaf `index`: per level l <
// levels, cur = compress(cur, sibling(l)) in the order bit l of index says,
// then cur = after_level(l + 1, cur) -- where a mixed-height tree injects
// (merkle_mixed.cpp), the identity for a plain one.
template <class Sibling, class AfterLevel>
Fr merkle_path_root(const P2Host& p2, Fr cur, size_t index, uint32_t levels, Sibling&& sibling,
                    AfterLevel&& after_level) {
    for (uint32_t l = 0; l < levels; ++l) {
        const Fr sib = sibling(l);
        cur = after_level(l + 1, ((index >> l) & 1) ? p2.compress(sib, cur) : p2.compress(cur, sib));
    }
    return cur;
}
inline Fr no_injection(uint32_t, const Fr& cur) { return cur; }
// A tree of ctx with `leaves` leaves over nmats device matrices heights[k] x
// widths[k], each filled from src[k] -- the caller's host or device memory as
// `mem` says, on the context's stream -- or, with src null, left for the
// caller to write; and its layers, yet to be hashed.  LSP_E_OOM when the
// device has no room.  (merkle_mixed.cpp)
std::unique_ptr<lsp_tree> new_tree(lsp_ctx* ctx, size_t leaves, size_t nmats, const size_t* heights,
                                   const size_t* widths, const lsp_fr* const* src, int mem);
// ---- merkle.cpp
// one per proof in flight, for the proof's whole duration (the tree tops share the host's cores)
struct ActiveProof {
    ActiveProof();
    ~ActiveProof();
};
// defers the tree-top uploads of one proof until flush_top_uploads; the
// destructor drops any left (an error path)
struct DeferTopUploads {
    lsp_ctx* ctx;
    explicit DeferTopUploads(lsp_ctx* c);
    ~DeferTopUploads();
};
void flush_top_uploads(lsp_ctx* ctx);
// the GPU's Poseidon2 peak, M permutations/s: register-resident chains, the
// best of several grid sizes (lsp_calibrate_poseidon2; the host slice's plan)
double calibrate_poseidon2(lsp_ctx* ctx);
// The host slice's plumbing (host_slice.hpp), shared by the two owners of a
// tree.  slice_stream_begin: the side stream, made to wait for all the main
// stream holds so far (what makes the tree's input); the caller queues the
// downloads of the slice's rows on it, then slice_stream_end records
// ctx->ev_slice behind them.
hipStream_t slice_stream_begin(lsp_ctx* ctx);
void slice_stream_end(lsp_ctx* ctx);
// out[i] = the sponge of row i of the n host matrices side by side, i in [i0, i1)
void host_hash_rows(const P2Host& p2, const Fr* const* rows, const size_t* width, size_t n, Fr* out, size_t i0,
                    size_t i1);
// the levels above `first` digests host[0, first) on the host pool; returns the
// end of the layers.  pairs (optional): the digests are made first, as
// compress(pairs[2i], pairs[2i+1])
size_t host_levels(lsp_ctx* ctx, Fr* host, size_t first, host_clock::time_point* t_first = nullptr,
                   const Fr* pairs = nullptr);
// root of a tree whose bottom subtrees live on comm's ranks (`local` = this
// rank's); `top` gets the host layers above the subtrees
Fr shard_root(lsp_ctx* ctx, Comm& comm, const Fr& local, std::vector<std::vector<Fr>>& top, const char* tag);
// coset LDE of an h x w device matrix with per-column shifts -> (h << added_bits) x w bit-reversed rows
// (the whole-matrix LdeRequest of the C API and the PCS)
void lde_device(lsp_ctx* ctx, const Fr* d_in, size_t h, size_t w, uint32_t added_bits, const Fr* shifts_host,
                Fr* d_out);
// TwoAdicSubgroupDft::coset_dft_batch / coset_idft_batch on device matrices (h x w row-major):
// coefficients -> evaluations on shift H_h stored bit-reversed, and natural-order evaluations -> coefficients
void coset_dft_device(lsp_ctx* ctx, const Fr* d_coef, size_t h, size_t w, const Fr& shift, Fr* d_out);
void coset_idft_device(lsp_ctx* ctx, const Fr* d_evals, size_t h, size_t w, const Fr& shift, Fr* d_out);
// the pending phase events of the last proof -> ctx->timings (prove.cpp)
void resolve_timings(lsp_ctx* ctx);
// Merkle levels of at most this many digests run on the host: the context's
// value, 256 while several proofs are in flight in the process, LSP_HOST_TREE_TOP
// over both
size_t host_tree_top(const lsp_ctx* ctx);
// leaves + every layer into `layers` (2*height - 1); returns the root
// top: the caller's host_tree_top (0: every level on the device)
// fold: when set, the leaves are the pairs of the FRI fold it describes (fused
// into the leaf kernel; m.ptr[0] receives the folded vector)
// side (optional): called once, after the tree's launches are issued and before
// the host waits for them, with an event on the context's stream that follows
// the leaves and the wide levels (every level of more than 2^15 digests): work
// queued behind it on another stream fills the chip beside the narrow levels
// and the host's tree top
// A big tree inside a lone proof (or any, under LSP_HOST_SLICE) has a host slice
// (host_slice.hpp): the pool hashes the last leaves >> k leaves and their
// subtree down to the layer of `top` digests while the GPU takes the prefix
Fr commit_device(lsp_ctx* ctx, const MatList& m, size_t height, Fr* layers, size_t top, const FoldSpec* fold = nullptr,
                 const std::function<void(hipEvent_t)>* side = nullptr);
// Mixed-height batches (merkle_mixed.cpp; U14).  A class = the matrices of one
// height, by the caller's indices in the caller's order; classes tallest first
// (p3's stable sort by height).  height_classes checks the batch: LSP_E_SIZE
// for a height that is no power of two or above 2^40 and for a matrix beyond
// 2^48 elements, LSP_E_ARG for no matrix, a width outside [1, 2^20] (MatList
// holds widths as 32 bits) or a ninth matrix in a class (MatList's limit).
struct HeightClass {
    size_t height;
    std::vector<size_t> idx;
};
std::vector<HeightClass> height_classes(const size_t* widths, const size_t* heights, size_t nmats);
// every class's row digests, then the levels from the leaves to the root with
// each class injected at the level of its height, all on the context's stream;
// mats: device matrices, by the caller's indices.  layers: 2 * cls[0].height - 1
// digests, the layers after injection.  Returns the root.
Fr commit_mixed_device(lsp_ctx* ctx, const std::vector<HeightClass>& cls, const Fr* const* mats, const size_t* widths,
                       Fr* layers);
// Mmcs::verify_batch of such a batch on the host: rows = one opened row per
// matrix in the caller's order, path = log2(cls[0].height) digests
bool verify_mixed_host(const lsp_ctx* ctx, const Fr& root, const std::vector<HeightClass>& cls, const size_t* widths,
                       size_t nmats, size_t index, const lsp_fr* rows, const lsp_fr* path);
// GrindingChallenger::grind(bits) on the device, re-checked on (and applied to) the host transcript (prove.cpp)
uint64_t grind_device(lsp_ctx* ctx, Challenger& ch, uint32_t bits);
// ---- fri.cpp: FRI, shared by the prover (prove.cpp) and the PCS (pcs.cpp)
struct FriRound {
    const Fr* vec;   // this rank's copy of the round's input (its slice when sharded)
    const Fr* tree;  // layers of this rank's (sub)tree
    size_t ml;       // leaves of that (sub)tree
    bool sharded;
    std::vector<std::vector<Fr>> top;
};
// The commit phase: per round the tree of the vector's pairs (the previous
// round's fold, with any roll-in, fused into its leaves), its root into `roots`
// and the transcript, beta out of it, and this round's fold left pending.  On
// comm's ranks each holds a contiguous slice of the vector until a slice is
// shorter than fri_shard_min; the last rounds run on the host once a round has
// at most host_tail leaves and no roll-in remains.
struct FriCommit {
    // the reduced-opening vector of `len` elements that rolls in where the
    // folded vector is as long (device memory), or nullptr
    using AddOfLen = std::function<const Fr*(size_t len)>;
    lsp_ctx* const ctx;
    Comm& comm;
    const uint32_t b, g;  // log2 of the ranks, this rank
    const size_t final_len;
    // policy, fixed here: LSP_HOST_TREE_TOP / LSP_FRI_HOST_TAIL / LSP_FRI_SHARD_MIN override the caller's values
    const size_t host_tree_top, host_tail, fri_shard_min;
    const AddOfLen add_of_len;
    std::vector<Fr>& roots;
    // the cursor: the current round's input (this rank's slice of a vector of
    // global length len), where the next fold goes (area + ao: the folds lie
    // back to back), the next tree (ftree + to) -- and the fold still owed:
    // round r's fold (by beta_r) runs fused into round r+1's leaf hashing
    const Fr* cur;
    Fr* area;
    Fr* ftree = nullptr;
    size_t len, ao = 0, to = 0;
    bool sharded;
    FoldSpec pend{};
    size_t pend_m = 0;  // folded values (this rank's slice)
    bool pending = false;
    std::vector<FriRound> rounds;

    // input: round 0's vector (this rank's n / comm.size elements of n);
    // fold_area: as much again, for the folded vectors
    FriCommit(lsp_ctx* ctx, Comm& comm, const Fr* input, Fr* fold_area, size_t n, std::vector<Fr>& roots,
              AddOfLen add_of_len, size_t host_tree_top, size_t host_tail);
    std::vector<Fr> commit(Challenger& ch);  // returns the final vector
    // span: log the prover's "divide_by_height" line; rehearsal: no degree check
    std::vector<Fr> final_poly(const std::vector<Fr>& fin, bool span, bool rehearsal) const;
    // one query's commit-phase openings below the rank subtrees: per round the
    // sibling's address and the path's; query_elems of them
    void push_query(std::vector<uint64_t>& ptrs, size_t idx) const;
    size_t query_elems() const;

  private:
    bool host_tail_fits() const;
    void replicate();
    void flush_fold();
    void fri_device_round(Challenger& ch);
    const Fr* fri_host_tail(Challenger& ch);
    size_t fri_host_round(Challenger& ch, Fr* v, Fr* lay);
};
// the addresses of the path of `leaf` in a tree of `leaves` leaves laid out at `layers`
void push_path(std::vector<uint64_t>& ptrs, const Fr* layers, size_t leaves, size_t leaf);
// the elements at ptrs (device addresses), gathered by one kernel, on the host
const Fr* gather_to_host(lsp_ctx* ctx, const std::vector<uint64_t>& ptrs);
// the verifier.  fold_row: TwoAdicFriGenericConfig::fold_row.  fri_replay: the
// roots into the transcript and the betas out of it, the final polynomial, the
// proof-of-work witness; 0, 6 (a witness beyond 64 bits) or 7 (refused).
// fri_check_query: one query's fold chain from `index` of the tallest vector
// (2^lmax) against the roots -- ro_of_log_height(l): the reduced opening that
// rolls in at height 2^l or nullptr; sib / path_len / path(k, l): round k's
// opening, called in wire order -- and the final polynomial; 0, 10 or 11
Fr fold_row(size_t index, uint32_t log_height, const Fr& beta, const Fr& e0, const Fr& e1);
// One matrix's term of a query's reduced opening at the LDE point x (both
// verifiers): over its points p and columns c,
// apow alpha^(p w + c) (row[c] - ys[p w + c]) / (x - zs[p]).  apow, the running
// power of alpha, leaves multiplied by alpha^(npts w).
inline Fr reduced_opening_term(const Fr* row, const Fr* ys, size_t w, const Fr* zs, size_t npts, const Fr& x,
                               const Fr& alpha, Fr& apow) {
    Fr term = fr_zero();
    for (size_t p = 0; p < npts; ++p) {
        Fr s = fr_zero();
        for (size_t c = 0; c < w; ++c) {
            s = fr_add(s, fr_mul(apow, fr_sub(row[c], ys[p * w + c])));
            apow = fr_mul(apow, alpha);
        }
        term = fr_add(term, fr_mul(s, fr_inv(fr_sub(x, zs[p]))));
    }
    return term;
}
int fri_replay(Challenger& ch, const lsp_ctx* ctx, const std::vector<Fr>& roots, const std::vector<Fr>& final_poly,
               const Fr& pow_w, std::vector<Fr>& betas);
int fri_check_query(const P2Host& p2, const std::vector<Fr>& roots, const std::vector<Fr>& betas,
                    const std::vector<Fr>& final_poly, uint32_t lmax, size_t index,
                    const std::function<const Fr*(uint32_t)>& ro_of_log_height,
                    const std::function<Fr(uint32_t)>& sib, const std::function<uint32_t(uint32_t)>& path_len,
                    const std::function<Fr(uint32_t, uint32_t)>& path);
// ---- pcs.cpp: TwoAdicFriPcs over batches of unequal heights
// One opening problem as commit, open and verify all see it: per batch the LDE
// heights and widths of its matrices in the caller's order, per matrix its points.
struct PcsRounds {
    struct Mat {
        size_t N, width;  // N: the LDE height
        std::vector<Fr> points;
    };
    std::vector<std::vector<Mat>> batches;
    size_t log_nmax = 0;  // of the tallest LDE over all batches (check sets it)
    // the refusals of U15, before any launch: LSP_E_ARG / LSP_E_SIZE
    void check(const lsp_ctx* ctx);
};
// the tree of the LDEs of n matrices heights[k] x widths[k] with domain shifts
// shifts[k] (nullptr: all one), read from the caller's host or device memory
std::unique_ptr<lsp_tree> pcs_commit(lsp_ctx* ctx, const lsp_fr* const* mats, const size_t* heights,
                                     const size_t* widths, const lsp_fr* shifts, size_t n, int mem, Fr* root);
// TwoAdicFriPcs::open of R.batches[b] = the matrices of trees[b]
std::unique_ptr<lsp_pcs_proof> pcs_open(lsp_ctx* ctx, const lsp_tree* const* trees, PcsRounds& R, Challenger& ch);
// 0 = accept, otherwise the failing check (host only).  commits: one root per batch
int pcs_verify_host(const lsp_ctx* ctx, const Fr* commits, PcsRounds& R, const uint8_t* b, size_t n, Challenger& ch);
std::vector<uint8_t> pcs_serialize(const lsp_pcs_proof& p);
// 0, or the check that refused the bytes (1: header, 5: body, 12: queries or trailing bytes)
int pcs_parse(const uint8_t* b, size_t n, lsp_pcs_proof& p);
// prep (optional): the committed preprocessed matrix -- a tree of ctx itself over
// exactly one matrix of height h << log_blowup (lsp_preprocess's, or an
// lsp_merkle_commit over a caller-made LDE); the proof then opens it too (LSPPRF03)
lsp_proof* prove_device(lsp_ctx* ctx, const Fr* d_trace, size_t h, size_t w, const Air& air, const Fr* pub,
                        size_t npub, const lsp_tree* prep = nullptr);
// p3-uni-stark check_constraints over the h x w trace (check.cpp): the device
// path (k_check.hip; d_trace on ctx's GPU) and the host loop fill the same
// report; list = the first `cap` violations in (row, constraint) order.
// prep (optional): the raw h x wp preprocessed matrix, where the trace is
struct CheckReport {
    lsp_check_summary s;
    std::vector<uint64_t> counts, first_rows;  // per constraint; first_rows UINT64_MAX = none
    std::vector<lsp_violation> list;
};
CheckReport check_constraints_device(lsp_ctx* ctx, const Fr* d_trace, size_t h, size_t w, const Air& air,
                                     const Fr* pub, size_t npub, size_t cap, const Fr* d_prep = nullptr,
                                     size_t wp = 0);
CheckReport check_constraints_host(const Fr* trace, size_t h, size_t w, const Air& air, const Fr* pub, size_t npub,
                                   size_t cap, const Fr* prep = nullptr, size_t wp = 0);
// "constraints had nonzero value on row R: constraint J (config C, <kind>[, table T]); N rows fail"
std::string check_failure_message(const Air& air, const CheckReport& r);
// one rank of a proof sharded over comm.size ranks (prove_device = 1 rank);
// every rank returns the same proof
lsp_proof* prove_shard(lsp_ctx* ctx, Comm& comm, const Fr* d_trace, size_t h, size_t w, const Air& air,
                       const Fr* pub, size_t npub, const lsp_tree* prep = nullptr);
// collective (every rank of comm): time an allgather of up to 256 MiB and this
// GPU's inverse NTT, agree on the minimum over the ranks (comm.ag_gbs,
// comm.intt_gelem_s; every rank's raw values in comm.calib_raw)
void calibrate_exchange(lsp_ctx* ctx, Comm& comm);
// this GPU's inverse-NTT rate (G elements/s) on an h x w matrix of seeded
// random elements, h = 2^log_h: median of `reps` after a warm-up, `before`
// ahead of each rep (may be empty)
double calibrate_intt(lsp_ctx* ctx, uint32_t log_h, size_t w, int reps, const std::function<void()>& before);
// the quotient-chunk broadcasts a sharded proof of h rows with q chunks issues
// on comm (either exchange choice): their count, bytes each, and their time
// at the calibrated allgather bandwidth (0 when uncalibrated)
struct QuotientExchange {
    size_t bcasts, bytes_each;
    double model_ms;
};
QuotientExchange quotient_exchange(const Comm& comm, size_t h, size_t q, uint32_t log_blowup);
// the inverse-NTT exchange a sharded proof of h x w (q quotient chunks) over
// comm makes: true = split by columns + an allgather of the coefficients,
// false = every rank inverts every column (LSP_SHARD_SPLIT_INTT=0/1 forces
// it); rank-identical
struct ExchangePlan {
    bool split;
    double allgather_ms, redundant_ms;  // the model's two costs (0 when uncalibrated)
    const char* reason;
};
ExchangePlan exchange_plan(const Comm& comm, size_t h, size_t w, size_t q, uint32_t log_blowup);
// proof wire format and field view (proof.cpp)
// pool (optional): the queries are written in parallel (the element
// conversions to canonical words are ~2/3 of a 2^19 proof's 10 K elements)
// reuse (optional): a buffer whose allocation the result takes over
std::vector<uint8_t> serialize(const lsp_proof& p, HostPool* pool = nullptr, std::vector<uint8_t>* reuse = nullptr);
lsp_proof* deserialize(const uint8_t* buf, size_t len);
// A freed proof's largest allocations -- its wire bytes (a fresh 324 KB vector
// per 2^19 proof is an mmap, page faults and an munmap) and its query records
// (~800 small vectors) -- go back to a small process-wide stock that the next
// proof's query assembly and serialization take from (proof.cpp)
void proof_release(lsp_proof* p);
std::vector<uint8_t> recycled_wire();
std::vector<lsp_query> recycled_queries();
void proof_view(const lsp_proof& p, lsp_proof_view* v);
// the preprocessed openings of an LSPPRF03 proof; LSP_E_STATE on an LSPPRF02 one
void proof_prep_view(const lsp_proof& p, lsp_proof_preprocessed_view* v);
lsp_proof* proof_from_view(const lsp_proof_view& v);
// communicators of a process-per-GPU sharded prove (comm_ext.cpp)
Comm* make_callback_comm(const lsp_comm_ops& ops);
void rccl_unique_id(uint8_t out[128]);
Comm* make_rccl_comm(const uint8_t id[128], int rank, int size);
// witness blocks on the device (witness.cpp): raw columns column-major in, rows
// written at out + i * ostride in witness_layout.hpp's order
void witness_permutation_device(lsp_ctx* ctx, const Fr* a, uint32_t na, const Fr* b, uint32_t nb, size_t n,
                                const Fr& alpha, const Fr& delta, Fr* out, size_t ostride);
void witness_lookup_device(lsp_ctx* ctx, const Fr* a, uint32_t na, const Fr* b, uint32_t nt, uint32_t nbc,
                           const Fr* afil, const Fr* bfil, size_t n, const Fr& alpha, const Fr& delta, Fr* out,
                           size_t ostride);
// CBOR RawPermutationTrace / RawLookupTrace (cbor.cpp).  raw_trace_columns: the
// columns resized to `height`, column-major in the block's raw order
lsp_raw_trace* parse_raw_trace(const uint8_t* buf, size_t len);
void raw_trace_shape(const lsp_raw_trace& t, size_t& height, size_t& width);
std::vector<Fr> raw_trace_columns(const lsp_raw_trace& t, size_t height);
// 0 = accept, otherwise the failing check (host CPU verifier).  prep_commit
// (optional) and prep_width: the preprocessed matrix's root and width, for an
// "LSPPRF03" proof (verify.cpp)
int verify_host(const lsp_ctx* ctx, const Air& air, const Fr* pub, size_t npub, const uint8_t* b, size_t n,
                const Fr* prep_commit = nullptr, uint32_t prep_width = 0);
}  // namespace lsp
