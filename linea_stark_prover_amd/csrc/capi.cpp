// extern "C" entry points of liblsp_hip.so (declared in include/lsp.h); the
// witness, raw-trace and trace-generator ones are in witness.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>

#include "capi_internal.hpp"
#include "comm.hpp"
#include "splitmix.hpp"

using namespace lsp;

thread_local std::string lsp::g_err;

#ifdef LSP_DEBUG_BOUNDS
// The debug build: every kernel translation unit's fault word after a C-ABI
// call (dbg_bounds.hpp), with its (file code, line) mapped back to a name
std::string lsp::bounds_fault_report() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return "";
    (void)hipDeviceSynchronize();  // the call's kernels are done (any stream)
    // a new kernel file adds one line here; a header with an LSP_BOUNDS, one name below
    static const struct {
        const char* tu;
        unsigned (*reader)();
    } tus[] = {{"k_ntt.hip", bounds_fault_k_ntt},         {"k_hash.hip", bounds_fault_k_hash},
               {"k_field.hip", bounds_fault_k_field},     {"k_quotient.hip", bounds_fault_k_quotient},
               {"k_open.hip", bounds_fault_k_open},       {"k_witness.hip", bounds_fault_k_witness},
               {"k_check.hip", bounds_fault_k_check},     {"k_merkle_inject.hip", bounds_fault_k_merkle_inject},
               {"k_fri.hip", bounds_fault_k_fri}};
    static const char* const headers[] = {"fr29.hpp", "k_common.hpp", "poseidon2_f29.hpp", "fr.hpp", "k_air_prog.hpp"};
    std::string out;
    for (const auto& t : tus) {
        const unsigned v = t.reader();
        if (!v) continue;
        std::string file = "file#" + std::to_string(v >> 16);
        for (const auto& u : tus)
            if (dbg::file_code(u.tu) == (v >> 16)) file = u.tu;
        for (const char* f : headers)
            if (dbg::file_code(f) == (v >> 16)) file = f;
        out += (out.empty() ? "" : "; ") + std::string("device bounds check failed at ") + file + ":" +
               std::to_string(v & 0xffffu) + " (kernels of " + t.tu + ")";
    }
    return out;
}

void lsp::dbg_check_after(const char* what) {
    const std::string bad = bounds_fault_report();
    if (!bad.empty()) throw LspError(LSP_E_STATE, bad + " after " + what);
}
#endif

// device input: either the caller's device pointer or a pool copy of host data.
// The host copy is one pageable hipMemcpyAsync: it moves a 2^19 x 8 trace at
// 56 GB/s, the PCIe link's rate -- the same as from pinned memory (57) or from
// the caller's buffer registered in place (57; 27 once the registration of a
// fresh buffer is counted), and faster than staging through a pinned ring
// filled by host threads (37-46): tools/ubench/h2d.hip, profiles/r05b_h2d.json,
// r05c_h2d.json; in-proof A/B tools/time_upload.py, profiles/r05c_time_upload.txt
const Fr* lsp::dev_in(lsp_ctx* ctx, const lsp_fr* p, size_t n, int mem, const char* name) {
    LSP_REQUIRE(p || n == 0, LSP_E_ARG, "null input pointer");
    if (mem == LSP_MEM_DEVICE) return reinterpret_cast<const Fr*>(p);
    LSP_REQUIRE(mem == LSP_MEM_HOST, LSP_E_ARG, "mem must be LSP_MEM_HOST or LSP_MEM_DEVICE");
    Fr* d = ctx->fbuf(name, n ? n : 1);
    if (n) LSP_HIP(hipMemcpyAsync(d, p, n * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    return d;
}

void lsp::need_gpu(lsp_ctx* ctx) {
    LSP_REQUIRE(ctx, LSP_E_ARG, "null ctx");
    LSP_REQUIRE(ctx->device != LSP_HOST_ONLY, LSP_E_STATE, "host-only context (LSP_HOST_ONLY) has no GPU");
    LSP_HIP(hipSetDevice(ctx->device));
}

namespace {
Fr* dev_out(lsp_ctx* ctx, lsp_fr* p, size_t n, int mem, const char* name) {
    LSP_REQUIRE(p || n == 0, LSP_E_ARG, "null output pointer");
    if (mem == LSP_MEM_DEVICE) return reinterpret_cast<Fr*>(p);
    return ctx->fbuf(name, n ? n : 1);
}
void finish_out(lsp_ctx* ctx, lsp_fr* p, const Fr* d, size_t n, int mem) {
    if (mem == LSP_MEM_HOST && n)
        LSP_HIP(hipMemcpyAsync(p, d, n * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
}

// n caller elements (public values, opened values) as Fr
std::vector<Fr> to_frs(const lsp_fr* p, size_t n) {
    std::vector<Fr> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = to_fr(p[i]);
    return v;
}
}  // namespace

extern "C" {

#ifdef LSP_DEBUG_BOUNDS
const char* lsp_version(void) { return "linea_stark_prover_amd 0.1 (gfx950, debug-bounds)"; }
#else
const char* lsp_version(void) { return "linea_stark_prover_amd 0.1 (gfx950)"; }
#endif

int lsp_debug_bounds_probe(lsp_ctx* ctx) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx, LSP_E_ARG, "null ctx");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
#ifndef LSP_DEBUG_BOUNDS
        throw LspError(LSP_E_STATE, "not a debug-bounds build (python -m linea_stark_prover_amd.build --debug-bounds)");
#else
        uint32_t* sink = (uint32_t*)ctx->buf("bounds_probe", 4 * sizeof(uint32_t));
        LSP_HIP(launch_bounds_probe(sink, ctx->stream));
        ctx->sync();  // guarded() then reports the probe's failed check as LSP_E_STATE
#endif
    });
}

int lsp_device_count(int* n) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(n, LSP_E_ARG, "null");
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
        *n = c;
    });
}

const char* lsp_last_error(const lsp_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int lsp_seeded_setup(uint64_t seed, uint32_t rounds_f, uint32_t rounds_p, lsp_fr* alpha, lsp_fr* delta,
                     lsp_fr* rc) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(alpha && delta && rc && rounds_f % 2 == 0, LSP_E_ARG, "bad seeded_setup arguments");
        SplitMix64 g{seed};
        *alpha = from_fr(g.fr());
        *delta = from_fr(g.fr());
        for (uint32_t i = 0; i < 3 * rounds_f + rounds_p; ++i) rc[i] = from_fr(g.fr());
    });
}

// The scalar helpers return nothing (the reference's field methods cannot
// fail); a null argument makes them a no-op instead of a fault.
void lsp_fr_from_canonical(const uint64_t in[4], lsp_fr* out) {
    if (!in || !out) return;
    lsp_fr t;
    std::memcpy(t.l, in, 32);
    *out = from_fr(fr_from_canonical(to_fr(t)));
}
void lsp_fr_to_canonical(const lsp_fr* in, uint64_t out[4]) {
    if (!in || !out) return;
    lsp_fr t = from_fr(fr_to_canonical(to_fr(*in)));
    std::memcpy(out, t.l, 32);
}
void lsp_fr_from_be_bytes_mod_order(const uint8_t* be, size_t n, lsp_fr* out) {
    if (!out || (!be && n)) return;
    // Horner over bytes: acc = acc * 256 + byte (mod r)
    const Fr b256 = fr_from_u64(256);
    Fr acc = fr_zero();
    for (size_t i = 0; i < n; ++i) acc = fr_add(fr_mul(acc, b256), fr_from_u64(be[i]));
    *out = from_fr(acc);
}
void lsp_fr_mul(const lsp_fr* a, const lsp_fr* b, lsp_fr* out) {
    if (a && b && out) *out = from_fr(fr_mul(to_fr(*a), to_fr(*b))); }
void lsp_fr_inv(const lsp_fr* a, lsp_fr* out) {
    if (a && out) *out = from_fr(fr_inv(to_fr(*a)));
}
void lsp_two_adic_generator(uint32_t bits, lsp_fr* out) {
    if (!out) return;
    if (bits > 47) bits = 47;
    *out = from_fr(host_two_adic_generator(bits));
}

int lsp_ctx_create(int device, const lsp_params* p, lsp_ctx** out) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(p && out && p->round_constants, LSP_E_ARG, "null params");
        LSP_REQUIRE(p->struct_size == sizeof(lsp_params), LSP_E_ARG,
                    "lsp_params.struct_size must be sizeof(lsp_params) of this header (caller built against "
                    "another lsp.h?)");
        LSP_REQUIRE(p->skip_log_degree <= 1 && p->skip_public_values <= 1 && p->observe_opened_values <= 1 &&
                        p->sample_bits_montgomery <= 1 && p->skip_final_poly <= 1,
                    LSP_E_ARG, "transcript switches are 0 or 1");
        LSP_REQUIRE(p->sbox_degree == 11 || p->sbox_degree == 17, LSP_E_ARG, "S-box degree must be 11 or 17");
        LSP_REQUIRE(p->rounds_f >= 2 && p->rounds_f % 2 == 0 && p->rounds_f <= 64 && p->rounds_p <= 256, LSP_E_ARG,
                    "bad round counts");
        LSP_REQUIRE(p->log_blowup >= 1 && p->log_blowup <= 8 && p->num_queries >= 1 && p->num_queries <= 1024 &&
                        p->proof_of_work_bits <= 32 && p->log_final_poly_len <= 8 &&
                        (p->public_degree == 0 || p->public_degree == 1),
                    LSP_E_ARG, "bad FRI parameters");
        auto c = std::make_unique<lsp_ctx>();
        c->device = device;
        c->p2.L = P2Layout{p->rounds_f, p->rounds_p, p->sbox_degree};
        const size_t nround = 3 * p->rounds_f + p->rounds_p;
        const size_t nrc = nround + P2_LIN_N;  // round constants, then M_E [9] and d [3]
        c->p2.rc.resize(nrc);
        for (size_t i = 0; i < nround; ++i) c->p2.rc[i] = to_fr(p->round_constants[i]);
        {
            // U2/U3: caller-set linear layers; the default values are stored
            // too, and gen_lin picks the generic path only when they differ
            static const uint32_t dm[9] = {2, 1, 1, 1, 2, 1, 1, 1, 2}, dd[3] = {1, 1, 2};
            bool gen = false;
            for (int k = 0; k < 9; ++k) {
                const Fr def = fr_from_u64(dm[k]);
                Fr v = def;
                if (p->external_mds) {
                    v = to_fr(p->external_mds[k]);
                    LSP_REQUIRE(fr_words_lt_mod(v), LSP_E_ARG, "external_mds entry not canonical");
                }
                gen |= !fr_eq(v, def);
                c->p2.rc[nround + k] = v;
            }
            for (int k = 0; k < 3; ++k) {
                const Fr def = fr_from_u64(dd[k]);
                Fr v = def;
                if (p->internal_diag) {
                    v = to_fr(p->internal_diag[k]);
                    LSP_REQUIRE(fr_words_lt_mod(v), LSP_E_ARG, "internal_diag entry not canonical");
                }
                gen |= !fr_eq(v, def);
                c->p2.rc[nround + 9 + k] = v;
            }
            c->p2.L.gen_lin = gen ? 1u : 0u;
        }
        if (ifma::available()) ifma::prepare(c->p2.rc, c->p2.rc8);
        if (device != LSP_HOST_ONLY) {  // LSP_HOST_ONLY: verifier-only context, no GPU touched
            int n = 0;
            if (hipGetDeviceCount(&n) != hipSuccess || n == 0) throw LspError(LSP_E_STATE, "no HIP device");
            LSP_REQUIRE(device >= 0 && device < n, LSP_E_ARG, "bad device index");
            LSP_HIP(hipSetDevice(device));
            LSP_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
            int lds = 0;  // LDS per workgroup (gfx950: 160 KiB): what the reduce-rows launch may use
            if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && lds > 0)
                c->lds_per_block = (size_t)lds;
            LSP_HIP(hipMalloc(&c->rc_dev, nrc * sizeof(Fr)));
            LSP_HIP(hipMemcpy(c->rc_dev, c->p2.rc.data(), nrc * sizeof(Fr), hipMemcpyHostToDevice));
            LSP_HIP(hipMalloc(&c->rc29_dev, nrc * sizeof(F29)));
            LSP_HIP(launch_rc_to_f29(c->rc_dev, c->rc29_dev, (uint32_t)nrc, c->stream));
            LSP_HIP(hipStreamSynchronize(c->stream));
        }
        c->log_blowup = p->log_blowup;
        c->log_final_poly_len = p->log_final_poly_len;
        c->num_queries = p->num_queries;
        c->pow_bits = p->proof_of_work_bits;
        c->public_degree = p->public_degree;
        c->transcript.log_degree = !p->skip_log_degree;
        c->transcript.public_values = !p->skip_public_values;
        c->transcript.opened_values = p->observe_opened_values != 0;
        c->transcript.mont_bits = p->sample_bits_montgomery != 0;
        c->transcript.final_poly = !p->skip_final_poly;
        *out = c.release();
    });
}

int lsp_ctx_destroy(lsp_ctx* ctx) {
    delete ctx;
    return LSP_OK;
}

int lsp_synchronize(lsp_ctx* ctx) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx, LSP_E_ARG, "null ctx");
        need_gpu(ctx);
        LSP_HIP(hipDeviceSynchronize());
    });
}

int lsp_dev_alloc(lsp_ctx* ctx, size_t bytes, void** dptr) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && dptr, LSP_E_ARG, "null");
        need_gpu(ctx);
        if (hipMalloc(dptr, bytes ? bytes : 1) != hipSuccess) {
            (void)hipGetLastError();
            throw LspError(LSP_E_OOM, "hipMalloc failed");
        }
    });
}
int lsp_dev_free(lsp_ctx* ctx, void* dptr) {
    return guarded(ctx, [&] {
        need_gpu(ctx);
        LSP_HIP(hipFree(dptr));
    });
}
int lsp_memcpy_h2d(lsp_ctx* ctx, void* dst, const void* src, size_t bytes) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && ((dst && src) || bytes == 0), LSP_E_ARG, "null memcpy argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        LSP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        ctx->sync();
    });
}
int lsp_memcpy_d2h(lsp_ctx* ctx, void* dst, const void* src, size_t bytes) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && ((dst && src) || bytes == 0), LSP_E_ARG, "null memcpy argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        LSP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
    });
}

int lsp_coset_lde_batch_shifts(lsp_ctx* ctx, const lsp_fr* in, size_t h, size_t w, uint32_t added_bits,
                               const lsp_fr* shifts, lsp_fr* out, int mem) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && shifts && w >= 1, LSP_E_ARG, "bad arguments");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        log2_exact(h);
        LSP_REQUIRE(added_bits <= 16, LSP_E_ARG, "added_bits too large");
        const size_t N = h << added_bits;
        std::vector<Fr> sh(w);
        for (size_t c = 0; c < w; ++c) sh[c] = to_fr(shifts[c]);
        const Fr* din = dev_in(ctx, in, h * w, mem, "api_in");
        Fr* dout = dev_out(ctx, out, N * w, mem, "api_out");
        lde_device(ctx, din, h, w, added_bits, sh.data(), dout);
        finish_out(ctx, out, dout, N * w, mem);
    });
}

int lsp_coset_lde_batch(lsp_ctx* ctx, const lsp_fr* in, size_t h, size_t w, uint32_t added_bits,
                        const lsp_fr* shift, lsp_fr* out, int mem) {
    if (!shift || w == 0) return LSP_E_ARG;
    std::vector<lsp_fr> sh(w, *shift);
    return lsp_coset_lde_batch_shifts(ctx, in, h, w, added_bits, sh.data(), out, mem);
}

int lsp_coset_dft_batch(lsp_ctx* ctx, const lsp_fr* coeffs, size_t h, size_t w, const lsp_fr* shift, lsp_fr* out,
                        int mem) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && w >= 1, LSP_E_ARG, "bad dft arguments");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        log2_exact(h);
        const Fr s = shift ? to_fr(*shift) : fr_one();
        const Fr* din = dev_in(ctx, coeffs, h * w, mem, "api_in");
        Fr* dout = dev_out(ctx, out, h * w, mem, "api_out");
        coset_dft_device(ctx, din, h, w, s, dout);
        finish_out(ctx, out, dout, h * w, mem);
    });
}

int lsp_coset_idft_batch(lsp_ctx* ctx, const lsp_fr* evals, size_t h, size_t w, const lsp_fr* shift, lsp_fr* out,
                         int mem) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && w >= 1, LSP_E_ARG, "bad idft arguments");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        log2_exact(h);
        const Fr s = shift ? to_fr(*shift) : fr_one();
        LSP_REQUIRE(!fr_is_zero(fr_to_canonical(s)), LSP_E_ARG, "coset shift must be nonzero");
        const Fr* din = dev_in(ctx, evals, h * w, mem, "api_in");
        Fr* dout = dev_out(ctx, out, h * w, mem, "api_out");
        coset_idft_device(ctx, din, h, w, s, dout);
        finish_out(ctx, out, dout, h * w, mem);
    });
}

int lsp_poseidon2_permute_batch(lsp_ctx* ctx, lsp_fr* states, size_t n, int mem) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx, LSP_E_ARG, "null ctx");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        Fr* d = const_cast<Fr*>(dev_in(ctx, states, 3 * n, mem, "api_in"));
        LSP_HIP(launch_permute(d, n, ctx->rc29_dev, ctx->p2.L, ctx->stream));
        finish_out(ctx, states, d, 3 * n, mem);
    });
}

int lsp_hash_rows(lsp_ctx* ctx, const lsp_fr* rows, size_t n, size_t w, lsp_fr* out, int mem) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx, LSP_E_ARG, "null ctx");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        const Fr* din = dev_in(ctx, rows, n * w, mem, "api_in");
        Fr* dout = dev_out(ctx, out, n, mem, "api_out");
        LSP_HIP(launch_hash_rows(one_mat(din, (uint32_t)w), n, dout, ctx->rc29_dev, ctx->p2.L, ctx->stream));
        finish_out(ctx, out, dout, n, mem);
    });
}

int lsp_merkle_commit(lsp_ctx* ctx, const lsp_fr* const* mats, const size_t* widths, size_t nmats, size_t height,
                      int mem, lsp_fr* root, lsp_tree** tree) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && mats && widths && root && nmats >= 1 && nmats <= 8, LSP_E_ARG,
                    "bad merkle_commit arguments (1..8 matrices)");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        log2_exact(height);
        for (size_t k = 0; k < nmats; ++k) LSP_REQUIRE(widths[k] >= 1 && mats[k], LSP_E_ARG, "bad matrix");
        const std::vector<size_t> heights(nmats, height);
        auto t = new_tree(ctx, height, nmats, heights.data(), widths, mats, mem);
        MatList m{};
        m.n = (uint32_t)nmats;
        for (size_t k = 0; k < nmats; ++k) {
            m.ptr[k] = t->mats[k];
            m.width[k] = (uint32_t)widths[k];
        }
        *root = from_fr(commit_device(ctx, m, height, t->layers, host_tree_top(ctx)));
        if (tree) *tree = t.release();
    });
}

int lsp_preprocess(lsp_ctx* ctx, const lsp_fr* cols, size_t h, size_t wp, int mem, lsp_fr* commit_out,
                   lsp_tree** out) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && cols && commit_out && out, LSP_E_ARG, "bad preprocess arguments");
        LSP_REQUIRE(wp >= 1 && wp <= (1u << 20), LSP_E_ARG, "preprocessed width outside [1, 2^20]");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        const uint32_t log_h = log2_exact(h);
        LSP_REQUIRE(h >= 2 && log_h + ctx->log_blowup <= 40, LSP_E_SIZE, "preprocessed height outside [2, 2^40 / blowup]");
        const size_t N = h << ctx->log_blowup;
        const Fr* din = dev_in(ctx, cols, h * wp, mem, "api_in");
        auto t = new_tree(ctx, N, 1, &N, &wp, nullptr, mem);
        // the LDE goes straight into the tree's buffer: no copy
        const std::vector<Fr> sh(wp, host_generator());
        lde_device(ctx, din, h, wp, ctx->log_blowup, sh.data(), t->mats[0]);
        *commit_out = from_fr(commit_device(ctx, one_mat(t->mats[0], (uint32_t)wp), N, t->layers, host_tree_top(ctx)));
        ctx->sync();  // the host-made tree top goes up asynchronously
        *out = t.release();
    });
}

int lsp_merkle_open(const lsp_tree* t, size_t index, lsp_fr* rows_out, lsp_fr* path_out) {
    if (!t) return LSP_E_ARG;
    lsp_ctx* ctx = t->ctx;
    return guarded(ctx, [&] {
        LSP_REQUIRE(index < t->height, LSP_E_ARG, "index out of range");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        // the commit's host-made top layers go up asynchronously on the context's
        // non-blocking stream; the copies below use the null stream
        LSP_HIP(hipStreamSynchronize(ctx->stream));
        size_t o = 0;
        if (rows_out)
            for (size_t k = 0; k < t->mats.size(); ++k) {
                LSP_HIP(hipMemcpy(rows_out + o, t->mats[k] + t->row_of(k, index) * t->widths[k],
                                  t->widths[k] * sizeof(Fr), hipMemcpyDeviceToHost));
                o += t->widths[k];
            }
        const TreeLayout lay{t->height};
        if (path_out)
            for (uint32_t l = 0, n = lay.levels(); l < n; ++l)
                LSP_HIP(hipMemcpy(path_out + l, t->layers + lay.sibling(l, index), sizeof(Fr), hipMemcpyDeviceToHost));
    });
}

int lsp_merkle_layer(const lsp_tree* t, uint32_t level, lsp_fr* out) {
    if (!t || !out) return LSP_E_ARG;
    lsp_ctx* ctx = t->ctx;
    return guarded(ctx, [&] {
        const TreeLayout lay{t->height};
        LSP_REQUIRE(level <= lay.levels(), LSP_E_ARG, "level out of range");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        // on the context's (non-blocking) stream: the host-made top layers are
        // uploaded asynchronously on it by the commit
        LSP_HIP(hipMemcpyAsync(out, t->layers + lay.offset(level), lay.len(level) * sizeof(Fr), hipMemcpyDeviceToHost,
                               ctx->stream));
        LSP_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int lsp_merkle_verify(const lsp_ctx* ctx, const lsp_fr* root, const size_t* widths, size_t nmats,
                      uint32_t log_height, size_t index, const lsp_fr* rows, const lsp_fr* path) {
    if (!ctx || !root || !widths || !rows || (log_height && !path)) return LSP_E_ARG;
    bool ok = false;
    const int rc = guarded(nullptr, [&] {
        size_t tot = 0;
        for (size_t k = 0; k < nmats; ++k) tot += widths[k];
        const std::vector<Fr> leaf = to_frs(rows, tot);
        const Fr got = merkle_path_root(
            ctx->p2, ctx->p2.hash(leaf.data(), tot), index, log_height, [&](uint32_t l) { return to_fr(path[l]); },
            no_injection);
        ok = fr_eq(got, to_fr(*root));
    });
    return rc != LSP_OK ? rc : ok ? LSP_OK : LSP_E_VERIFY;
}

int lsp_merkle_commit_mixed(lsp_ctx* ctx, const lsp_fr* const* mats, const size_t* widths, const size_t* heights,
                            size_t nmats, int mem, lsp_fr* root, lsp_tree** tree) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && mats && widths && heights && root, LSP_E_ARG, "bad merkle_commit_mixed arguments");
        LSP_REQUIRE(mem == LSP_MEM_HOST || mem == LSP_MEM_DEVICE, LSP_E_ARG,
                    "mem must be LSP_MEM_HOST or LSP_MEM_DEVICE");
        const std::vector<HeightClass> cls = height_classes(widths, heights, nmats);
        for (size_t k = 0; k < nmats; ++k) LSP_REQUIRE(mats[k], LSP_E_ARG, "null matrix");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        auto t = new_tree(ctx, cls[0].height, nmats, heights, widths, mats, mem);
        *root = from_fr(commit_mixed_device(ctx, cls, t->mats.data(), widths, t->layers));
        if (tree) *tree = t.release();
    });
}

int lsp_merkle_verify_mixed(const lsp_ctx* ctx, const lsp_fr* root, const size_t* widths, const size_t* heights,
                            size_t nmats, size_t index, const lsp_fr* rows, const lsp_fr* path) {
    bool ok = false;
    const int rc = guarded(nullptr, [&] {
        LSP_REQUIRE(ctx && root && widths && heights && rows, LSP_E_ARG, "bad merkle_verify_mixed arguments");
        const std::vector<HeightClass> cls = height_classes(widths, heights, nmats);
        LSP_REQUIRE(index < cls[0].height, LSP_E_ARG, "index out of range");
        LSP_REQUIRE(path || cls[0].height == 1, LSP_E_ARG, "null path");
        ok = verify_mixed_host(ctx, to_fr(*root), cls, widths, nmats, index, rows, path);
    });
    return rc != LSP_OK ? rc : ok ? LSP_OK : LSP_E_VERIFY;
}

int lsp_tree_dims(const lsp_tree* t, size_t* heights, size_t* widths, size_t cap, size_t* n) {
    if (!t) return LSP_E_ARG;
    const size_t nm = t->widths.size();
    if (n) *n = nm;
    for (size_t k = 0; k < nm && k < cap; ++k) {
        if (heights) heights[k] = t->heights[k];
        if (widths) widths[k] = t->widths[k];
    }
    return LSP_OK;
}

int lsp_tree_free(lsp_tree* t) {
    delete t;
    return LSP_OK;
}

// ------------------------------------------------------------------ Pcs
int lsp_challenger_create(const lsp_ctx* ctx, lsp_challenger** out) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(ctx && out, LSP_E_ARG, "bad challenger_create arguments");
        *out = nullptr;
        *out = new lsp_challenger(ctx);
    });
}

extern "C++" {
namespace {
lsp_challenger* live(lsp_challenger* ch) {
    LSP_REQUIRE(ch && ch->tag == lsp_challenger::TAG, LSP_E_ARG, "not a challenger handle");
    return ch;
}
const lsp_pcs_proof* live(const lsp_pcs_proof* p) {
    LSP_REQUIRE(p && p->tag == lsp_pcs_proof::TAG, LSP_E_ARG, "not a PCS proof handle");
    return p;
}
// the flat arguments of lsp_pcs_open / lsp_pcs_verify as PcsRounds, checked (U15's refusals)
PcsRounds pcs_rounds(const lsp_ctx* ctx, size_t nbatches, const std::function<size_t(size_t)>& nmats,
                     const std::function<std::pair<size_t, size_t>(size_t, size_t)>& dims, const size_t* npoints,
                     const lsp_fr* points) {
    PcsRounds R;
    LSP_REQUIRE(nbatches >= 1 && nbatches <= (1u << 16) && npoints, LSP_E_ARG, "a PCS opening needs 1 .. 2^16 batches");
    R.batches.resize(nbatches);
    size_t km = 0, kp = 0;
    for (size_t b = 0; b < nbatches; ++b) {
        const size_t nm = nmats(b);
        LSP_REQUIRE(nm >= 1 && nm <= (1u << 16), LSP_E_ARG, "a batch needs 1 .. 2^16 matrices");
        for (size_t k = 0; k < nm; ++k, ++km) {
            PcsRounds::Mat m;
            std::tie(m.N, m.width) = dims(b, k);
            LSP_REQUIRE(npoints[km] <= (1u << 16), LSP_E_ARG, "more than 2^16 points on a matrix");
            LSP_REQUIRE(npoints[km] == 0 || points, LSP_E_ARG, "null points");
            for (size_t p = 0; p < npoints[km]; ++p) m.points.push_back(to_fr(points[kp++]));
            R.batches[b].push_back(std::move(m));
        }
    }
    R.check(ctx);
    return R;
}
}  // namespace
}

int lsp_challenger_observe(lsp_challenger* ch, const lsp_fr* values, size_t n) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(values, LSP_E_ARG, "null values");
        Challenger& c = live(ch)->ch;
        for (size_t i = 0; i < n; ++i) c.observe(to_fr(values[i]));
    });
}

int lsp_challenger_sample(lsp_challenger* ch, lsp_fr* out) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(out, LSP_E_ARG, "null output");
        *out = from_fr(live(ch)->ch.sample());
    });
}

int lsp_challenger_sample_bits(lsp_challenger* ch, uint32_t bits, uint64_t* out) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(out && bits <= 64, LSP_E_ARG, "bad sample_bits arguments");
        *out = live(ch)->ch.sample_bits(bits);
    });
}

int lsp_challenger_free(lsp_challenger* ch) {
    return guarded(nullptr, [&] {
        live(ch)->tag = 0;
        delete ch;
    });
}

int lsp_pcs_commit(lsp_ctx* ctx, const lsp_fr* const* mats, const size_t* heights, const size_t* widths,
                   const lsp_fr* shifts, size_t n, int mem, lsp_fr* commit_out, lsp_tree** out) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && mats && heights && widths && commit_out && out, LSP_E_ARG, "bad pcs_commit arguments");
        LSP_REQUIRE(mem == LSP_MEM_HOST || mem == LSP_MEM_DEVICE, LSP_E_ARG,
                    "mem must be LSP_MEM_HOST or LSP_MEM_DEVICE");
        std::lock_guard<std::mutex> g(ctx->mu);
        Fr root;
        auto t = pcs_commit(ctx, mats, heights, widths, shifts, n, mem, &root);
        *commit_out = from_fr(root);
        *out = t.release();
    });
}

int lsp_pcs_open(lsp_ctx* ctx, const lsp_tree* const* trees, size_t ntrees, const size_t* npoints, const lsp_fr* points,
                 lsp_challenger* challenger, lsp_pcs_proof** out) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && trees && npoints && out, LSP_E_ARG, "bad pcs_open arguments");
        Challenger& ch = live(challenger)->ch;
        *out = nullptr;
        for (size_t b = 0; b < ntrees && b < (1u << 16); ++b)
            LSP_REQUIRE(trees[b] && trees[b]->ctx == ctx, LSP_E_ARG, "a tree is null or belongs to another context");
        std::lock_guard<std::mutex> g(ctx->mu);
        PcsRounds R = pcs_rounds(
            ctx, ntrees, [&](size_t b) { return trees[b]->mats.size(); },
            [&](size_t b, size_t k) { return std::make_pair(trees[b]->heights[k], trees[b]->widths[k]); }, npoints,
            points);
        need_gpu(ctx);
        *out = pcs_open(ctx, trees, R, ch).release();
    });
}

int lsp_pcs_proof_opened_values(const lsp_pcs_proof* proof, const lsp_fr** values, size_t* n) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(values && n, LSP_E_ARG, "null output");
        const lsp_pcs_proof* p = live(proof);
        std::lock_guard<std::mutex> g(p->cache_mu);
        if (p->ys_view.size() != p->ys.size())
            for (const Fr& y : p->ys) p->ys_view.push_back(from_fr(y));
        *values = p->ys_view.data();
        *n = p->ys_view.size();
    });
}

int lsp_pcs_proof_serialize(const lsp_pcs_proof* proof, uint8_t* buf, size_t cap, size_t* len) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(len, LSP_E_ARG, "null length");
        const std::vector<uint8_t> b = pcs_serialize(*live(proof));
        *len = b.size();
        if (buf) {
            LSP_REQUIRE(cap >= b.size(), LSP_E_ARG, "buffer too small");
            std::memcpy(buf, b.data(), b.size());
        }
    });
}

int lsp_pcs_proof_deserialize(const uint8_t* buf, size_t len, lsp_pcs_proof** out) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(buf && out, LSP_E_ARG, "null");
        *out = nullptr;
        auto p = std::make_unique<lsp_pcs_proof>();
        const int bad = pcs_parse(buf, len, *p);
        LSP_REQUIRE(bad == 0, LSP_E_ARG, "not an LSPPCS01 proof (check " + std::to_string(bad) + ")");
        *out = p.release();
    });
}

int lsp_pcs_proof_free(lsp_pcs_proof* proof) {
    return guarded(nullptr, [&] {
        live(proof);
        proof->tag = 0;
        delete proof;
    });
}

int lsp_pcs_verify(const lsp_ctx* ctx, const lsp_fr* commits, size_t nbatches, const size_t* nmats,
                   const size_t* heights, const size_t* widths, const size_t* npoints, const lsp_fr* points,
                   const uint8_t* proof, size_t len, lsp_challenger* challenger, int* failed_check) {
    int rc = LSP_OK;
    const int g = guarded(nullptr, [&] {
        LSP_REQUIRE(ctx && commits && nmats && heights && widths && npoints && proof, LSP_E_ARG,
                    "bad pcs_verify arguments");
        Challenger& ch = live(challenger)->ch;
        if (failed_check) *failed_check = 0;
        const uint32_t lb = ctx->log_blowup;
        std::vector<size_t> first(1, 0);  // batch b's matrices start at first[b] in the flat arrays
        PcsRounds R = pcs_rounds(
            ctx, nbatches,
            [&](size_t b) {
                first.push_back(first[b] + std::min<size_t>(nmats[b], 1u << 16));
                return nmats[b];
            },
            [&](size_t b, size_t k) {
                const size_t h = heights[first[b] + k];
                LSP_REQUIRE(h <= (((size_t)1 << 40) >> lb), LSP_E_SIZE, "matrix height beyond 2^40 / blowup");
                return std::make_pair(h << lb, widths[first[b] + k]);
            },
            npoints, points);
        const std::vector<Fr> roots = to_frs(commits, nbatches);
        const int v = pcs_verify_host(ctx, roots.data(), R, proof, len, ch);
        if (v != 0) {
            g_err = "PCS proof rejected at check " + std::to_string(v);
            if (failed_check) *failed_check = v;
            rc = LSP_E_VERIFY;
        }
    });
    return g != LSP_OK ? g : rc;
}

int lsp_fri_fold(lsp_ctx* ctx, const lsp_fr* v, size_t len, const lsp_fr* beta, lsp_fr* out, int mem) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && beta && len >= 2, LSP_E_ARG, "bad fri_fold arguments");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        const uint32_t lg = log2_exact(len);
        const size_t m = len / 2;
        const Fr* din = dev_in(ctx, v, len, mem, "api_in");
        Fr* dout = dev_out(ctx, out, m, mem, "api_out");
        FoldSpec f = fold_spec(ctx, lg - 1, 0, to_fr(*beta));
        f.v = din;
        f.vout = dout;
        fri_fold(ctx, f, m);
        finish_out(ctx, out, dout, m, mem);
    });
}

void lsp_fri_fold_row(size_t index, uint32_t log_height, const lsp_fr* beta, const lsp_fr* e0, const lsp_fr* e1,
                      lsp_fr* out) {
    if (!beta || !e0 || !e1 || !out) return;
    *out = from_fr(fold_row(index, log_height, to_fr(*beta), to_fr(*e0), to_fr(*e1)));
}

int lsp_log_quotient_degree(const int32_t* air, size_t air_len, int32_t public_degree, uint32_t* log_q) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(log_q, LSP_E_ARG, "null");
        *log_q = Air::parse(air, air_len).log_quotient_degree(public_degree);
    });
}

// lsp_quotient_values, and with a preprocessed LDE (prep_lde, wp) lsp_quotient_values_preprocessed
extern "C++" {
namespace {
int quotient_values(lsp_ctx* ctx, const lsp_fr* lde, size_t h, size_t w, const lsp_fr* prep_lde, size_t wp,
                    const int32_t* air, size_t air_len, const lsp_fr* pubv, size_t npub, const lsp_fr* alpha,
                    lsp_fr* out, int mem) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && alpha && pubv && npub >= 2, LSP_E_ARG, "bad quotient arguments");
        LSP_REQUIRE(wp <= (1u << 20), LSP_E_ARG, "preprocessed width past 2^20");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        const Air A = Air::parse(air, air_len);
        A.require_fits(w, npub, wp);
        const uint32_t log_h = log2_exact(h), log_q = A.log_quotient_degree(ctx->public_degree);
        const uint32_t logQ = log_h + log_q;
        LSP_REQUIRE(log_q <= ctx->log_blowup, LSP_E_ARG, "quotient degree exceeds the blowup");
        const size_t N = h << ctx->log_blowup, Q = (size_t)1 << logQ;
        const Fr* dlde = dev_in(ctx, lde, N * w, mem, "api_in");
        const Fr* dprep = wp ? dev_in(ctx, prep_lde, N * wp, mem, "api_prep") : nullptr;
        Fr* dout = dev_out(ctx, out, Q, mem, "api_out");
        QuotientArgs qa;
        const std::vector<Fr> pub = to_frs(pubv, npub);
        quotient_domain(ctx, log_h, log_q, 0, 0, Q, A, pub.data(), npub, qa);
        qa.lde = dlde;
        qa.w = (uint32_t)w;
        qa.alpha = to_fr(*alpha);
        qa.out = dout;
        qa.lde_rows = N;
        if (A.has_prog) {  // (only a program reads it)
            qa.prep = dprep;
            qa.wp = (uint32_t)wp;
        }
        LSP_HIP(launch_quotient(qa, ctx->stream));
        finish_out(ctx, out, dout, Q, mem);
    });
}
}  // namespace
}  // extern "C++"

int lsp_quotient_values(lsp_ctx* ctx, const lsp_fr* lde, size_t h, size_t w, const int32_t* air, size_t air_len,
                        const lsp_fr* pubv, size_t npub, const lsp_fr* alpha, lsp_fr* out, int mem) {
    return quotient_values(ctx, lde, h, w, nullptr, 0, air, air_len, pubv, npub, alpha, out, mem);
}

int lsp_quotient_values_preprocessed(lsp_ctx* ctx, const lsp_fr* lde, size_t h, size_t w, const lsp_fr* prep_lde,
                                     size_t wp, const int32_t* air, size_t air_len, const lsp_fr* pubv, size_t npub,
                                     const lsp_fr* alpha, lsp_fr* out, int mem) {
    if (!prep_lde || wp == 0) {
        (ctx ? ctx->err : g_err) = "a preprocessed LDE needs a pointer and a width";
        return LSP_E_ARG;
    }
    return quotient_values(ctx, lde, h, w, prep_lde, wp, air, air_len, pubv, npub, alpha, out, mem);
}

extern "C++" {
namespace {
// The open stage divides by z - x for every x of the coset shift * H_N: a
// point on the coset (z^N = shift^N) has no inverse denominators, and p3
// panics there.  Two host powers, before anything is launched.
void require_off_coset(const Fr& shift, const Fr* points, size_t npoints, size_t N) {
    LSP_REQUIRE(!fr_is_zero(fr_to_canonical(shift)), LSP_E_ARG, "coset shift must be nonzero");
    const Fr sN = fr_pow_u64(shift, N);
    for (size_t p = 0; p < npoints; ++p)
        LSP_REQUIRE(!fr_eq(fr_pow_u64(points[p], N), sN), LSP_E_ARG, "a point lies on the coset");
}
}  // namespace
}

int lsp_interpolate_coset(lsp_ctx* ctx, const lsp_fr* lde_bitrev, size_t h, size_t w, const lsp_fr* shift,
                          const lsp_fr* z, lsp_fr* ys_out, int mem) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && shift && z && ys_out && w >= 1, LSP_E_ARG, "bad interpolate arguments");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        const uint32_t logh = log2_exact(h);
        const Fr S = to_fr(*shift), Z = to_fr(*z);
        require_off_coset(S, &Z, 1, h);
        const Fr* dm = dev_in(ctx, lde_bitrev, h * w, mem, "api_in");
        Fr* inv = ctx->fbuf("o_invz", h);
        Fr* sums = ctx->fbuf("o_sums", w);
        open_denominators(ctx, Z, S, logh, 0, h, inv);
        barycentric_sums(ctx, dm, (uint32_t)w, h, inv, S, logh, 0, sums);
        std::vector<Fr> hs(w);
        LSP_HIP(hipMemcpyAsync(hs.data(), sums, w * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        const Fr f = CosetFactor(S, h, false).at(Z);
        for (size_t c = 0; c < w; ++c) ys_out[c] = from_fr(fr_mul(hs[c], f));
    });
}

int lsp_host_compress_batch(const lsp_ctx* ctx, const lsp_fr* pairs, size_t n, lsp_fr* out) {
    return guarded(const_cast<lsp_ctx*>(ctx), [&] {
        LSP_REQUIRE(ctx && (pairs || n == 0) && (out || n == 0), LSP_E_ARG, "bad host_compress arguments");
        std::vector<Fr> in(2 * n), o(n);
        for (size_t i = 0; i < 2 * n; ++i) in[i] = to_fr(pairs[i]);
        ctx->p2.compress_range(in.data(), o.data(), 0, n);
        for (size_t i = 0; i < n; ++i) out[i] = from_fr(o[i]);
    });
}

int lsp_host_hash_rows(const lsp_ctx* ctx, const lsp_fr* rows, size_t n, size_t w, lsp_fr* out) {
    return guarded(const_cast<lsp_ctx*>(ctx), [&] {
        LSP_REQUIRE(ctx && w >= 1 && (rows || n == 0) && (out || n == 0), LSP_E_ARG, "bad host_hash_rows arguments");
        std::vector<Fr> in(n * w), o(n);
        for (size_t i = 0; i < n * w; ++i) in[i] = to_fr(rows[i]);
        ctx->p2.hash_range(in.data(), w, o.data(), 0, n);
        for (size_t i = 0; i < n; ++i) out[i] = from_fr(o[i]);
    });
}

int lsp_batch_inverse(lsp_ctx* ctx, const lsp_fr* in, size_t n, lsp_fr* out, int mem) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx, LSP_E_ARG, "null ctx");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        const Fr* din = dev_in(ctx, in, n, mem, "api_in");
        Fr* dout = dev_out(ctx, out, n, mem, "api_out");
        LSP_REQUIRE(din != dout, LSP_E_ARG, "batch_inverse cannot run in place");
        LSP_HIP(launch_batch_inverse(din, dout, n, ctx->stream, ctx->bi_scratch(n)));
        finish_out(ctx, out, dout, n, mem);
    });
}

int lsp_inverse_denominators(lsp_ctx* ctx, const lsp_fr* points, size_t npoints, uint32_t log_n, const lsp_fr* shift,
                             lsp_fr* out, int mem) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && points && shift && npoints >= 1, LSP_E_ARG, "bad inverse_denominators arguments");
        LSP_REQUIRE(log_n <= 40, LSP_E_SIZE, "log_n too large");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        const size_t N = (size_t)1 << log_n;
        const std::vector<Fr> pts = to_frs(points, npoints);
        require_off_coset(to_fr(*shift), pts.data(), npoints, N);
        Fr* dout = dev_out(ctx, out, npoints * N, mem, "api_out");
        for (size_t p = 0; p < npoints; ++p)
            open_denominators(ctx, pts[p], to_fr(*shift), log_n, 0, N, dout + p * N);
        finish_out(ctx, out, dout, npoints * N, mem);
    });
}

int lsp_open_reduce(lsp_ctx* ctx, const lsp_fr* mat, size_t n, size_t w, const lsp_fr* inv_denoms, const lsp_fr* ys,
                    size_t npoints, const lsp_fr* alpha, lsp_fr* alpha_pow_offset, lsp_fr* ro, int mem) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && ys && alpha && alpha_pow_offset && ro && npoints >= 1 && w >= 1 && n >= 1, LSP_E_ARG,
                    "bad open_reduce arguments");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        const Fr* dm = dev_in(ctx, mat, n * w, mem, "api_in");
        const Fr* dinv = dev_in(ctx, inv_denoms, npoints * n, mem, "api_in2");
        Fr* dro = const_cast<Fr*>(dev_in(ctx, ro, n, mem, "api_out"));
        const std::vector<Fr> y = to_frs(ys, npoints * w);
        Fr off = to_fr(*alpha_pow_offset);
        reduce_matrix(ctx, dm, n, w, dinv, y.data(), npoints, to_fr(*alpha), off, dro, "api_coef");
        finish_out(ctx, ro, dro, n, mem);
        *alpha_pow_offset = from_fr(off);
    });
}

int lsp_prove(lsp_ctx* ctx, const lsp_fr* trace, size_t h, size_t w, const int32_t* air, size_t air_len,
              const lsp_fr* pubv, size_t npub, int mem, lsp_proof** out) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && out && pubv, LSP_E_ARG, "bad prove arguments");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        const Air A = Air::parse(air, air_len);
        const std::vector<Fr> pub = to_frs(pubv, npub);
        const Fr* din = dev_in(ctx, trace, h * w, mem, "trace_in");
        // the reference's debug-build check_constraints, opt-in (read per call, as LSP_QUOTIENT_ORDER is)
        if (const char* e = std::getenv("LSP_CHECK_CONSTRAINTS")) {
            if (e[0] == '1' && !e[1]) {
                const CheckReport r = check_constraints_device(ctx, din, h, w, A, pub.data(), npub, 0);
                if (r.s.failed_rows) throw LspError(LSP_E_CONSTRAINT, check_failure_message(A, r));
            }
        }
        *out = prove_device(ctx, din, h, w, A, pub.data(), npub);
    });
}

int lsp_prove_preprocessed(lsp_ctx* ctx, const lsp_fr* trace, size_t h, size_t w, const lsp_tree* prep,
                           const int32_t* air, size_t air_len, const lsp_fr* pubv, size_t npub, int mem,
                           lsp_proof** out) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && out && pubv && prep, LSP_E_ARG, "bad prove arguments");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        const Air A = Air::parse(air, air_len);
        const std::vector<Fr> pub = to_frs(pubv, npub);
        const Fr* din = dev_in(ctx, trace, h * w, mem, "trace_in");
        // (LSP_CHECK_CONSTRAINTS is not applied here: the tree holds the LDE, not the raw columns)
        *out = prove_device(ctx, din, h, w, A, pub.data(), npub, prep);
    });
}

// ---------------------------------------------------- check_constraints
int lsp_air_num_constraints(const int32_t* air, size_t air_len, uint32_t* n) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(n, LSP_E_ARG, "null");
        *n = Air::parse(air, air_len).num_constraints();
    });
}

int lsp_air_constraint_degree(const int32_t* air, size_t air_len, int32_t public_degree, uint32_t j,
                              uint32_t* degree) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(degree, LSP_E_ARG, "null");
        LSP_REQUIRE(public_degree >= 0 && public_degree <= 1024, LSP_E_ARG, "public_degree outside [0, 1024]");
        const std::vector<int> d = Air::parse(air, air_len).degrees(public_degree);
        LSP_REQUIRE(j < d.size(), LSP_E_ARG, "constraint index past the AIR's last constraint");
        *degree = (uint32_t)d[j];
    });
}

int lsp_air_constraint_info(const int32_t* air, size_t air_len, uint32_t j, uint32_t* config, int32_t* type,
                            int32_t* kind, int32_t* table) {
    return guarded(nullptr, [&] {
        const Air::ConsInfo ci = Air::parse(air, air_len).constraint_info(j);
        if (config) *config = ci.config;
        if (type) *type = ci.type;
        if (kind) *kind = ci.kind;
        if (table) *table = ci.table;
    });
}

// lsp_check_constraints, and with the raw preprocessed matrix (prep, wp) lsp_check_constraints_preprocessed
extern "C++" {
namespace {
int check_constraints(lsp_ctx* ctx, const lsp_fr* trace, size_t h, size_t w, const lsp_fr* prep, size_t wp,
                      const int32_t* air, size_t air_len, const lsp_fr* pubv, size_t npub, int mem,
                      lsp_check_summary* summary, uint64_t* counts, uint64_t* first_rows, lsp_violation* list,
                      size_t cap, size_t* nlist) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(wp <= (1u << 20), LSP_E_ARG, "preprocessed width past 2^20");
        LSP_REQUIRE(ctx && trace && pubv && summary, LSP_E_ARG, "bad check_constraints arguments");
        LSP_REQUIRE(cap == 0 || (list && nlist), LSP_E_ARG, "cap > 0 needs list and nlist");
        LSP_REQUIRE(mem == LSP_MEM_HOST || mem == LSP_MEM_DEVICE, LSP_E_ARG,
                    "mem must be LSP_MEM_HOST or LSP_MEM_DEVICE");
        LSP_REQUIRE(npub >= 2, LSP_E_ARG, "public values must hold [alpha, delta]");
        LSP_REQUIRE(h && !(h & (h - 1)), LSP_E_ARG, "trace height must be a power of two");
        std::lock_guard<std::mutex> g(ctx->mu);
        const Air A = Air::parse(air, air_len);
        A.require_fits(w, npub, wp);
        const std::vector<Fr> pub = to_frs(pubv, npub);
        CheckReport r;
        if (ctx->device == LSP_HOST_ONLY && mem == LSP_MEM_HOST) {
            // the host twin: a host-only context checks host memory (never a fallback on a GPU context)
            static_assert(sizeof(Fr) == sizeof(lsp_fr), "lsp_fr is Fr's words");
            std::vector<Fr> t(h * w);
            std::memcpy(t.data(), trace, t.size() * sizeof(Fr));
            std::vector<Fr> pm(h * wp);
            if (wp) std::memcpy(pm.data(), prep, pm.size() * sizeof(Fr));
            r = check_constraints_host(t.data(), h, w, A, pub.data(), npub, cap, wp ? pm.data() : nullptr, wp);
        } else {
            need_gpu(ctx);
            const Fr* din = dev_in(ctx, trace, h * w, mem, "trace_in");
            const Fr* dprep = wp ? dev_in(ctx, prep, h * wp, mem, "prep_in") : nullptr;
            r = check_constraints_device(ctx, din, h, w, A, pub.data(), npub, cap, dprep, wp);
        }
        *summary = r.s;
        if (counts) std::copy(r.counts.begin(), r.counts.end(), counts);
        if (first_rows) std::copy(r.first_rows.begin(), r.first_rows.end(), first_rows);
        if (nlist) *nlist = r.list.size();
        if (cap) std::copy(r.list.begin(), r.list.end(), list);
    });
}
}  // namespace
}  // extern "C++"

int lsp_check_constraints(lsp_ctx* ctx, const lsp_fr* trace, size_t h, size_t w, const int32_t* air, size_t air_len,
                          const lsp_fr* pubv, size_t npub, int mem, lsp_check_summary* summary, uint64_t* counts,
                          uint64_t* first_rows, lsp_violation* list, size_t cap, size_t* nlist) {
    return check_constraints(ctx, trace, h, w, nullptr, 0, air, air_len, pubv, npub, mem, summary, counts, first_rows,
                             list, cap, nlist);
}

int lsp_check_constraints_preprocessed(lsp_ctx* ctx, const lsp_fr* trace, size_t h, size_t w, const lsp_fr* prep,
                                       size_t wp, const int32_t* air, size_t air_len, const lsp_fr* pubv, size_t npub,
                                       int mem, lsp_check_summary* summary, uint64_t* counts, uint64_t* first_rows,
                                       lsp_violation* list, size_t cap, size_t* nlist) {
    if (!prep || wp == 0) {
        (ctx ? ctx->err : g_err) = "a preprocessed matrix needs a pointer and a width";
        return LSP_E_ARG;
    }
    return check_constraints(ctx, trace, h, w, prep, wp, air, air_len, pubv, npub, mem, summary, counts, first_rows,
                             list, cap, nlist);
}

// ------------------------------------------------------- sharded prove
struct lsp_group {
    std::vector<lsp_ctx*> ctxs;
};

int lsp_group_create(lsp_ctx* const* ctxs, int n, lsp_group** out) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(ctxs && out && n >= 1 && (n & (n - 1)) == 0, LSP_E_ARG, "a group is 2^b contexts");
        auto* grp = new lsp_group();
        grp->ctxs.assign(ctxs, ctxs + n);
        for (lsp_ctx* c : grp->ctxs) {
            if (!c || c->device == LSP_HOST_ONLY) {
                delete grp;
                throw LspError(LSP_E_ARG, "every group member needs a GPU context");
            }
        }
        // peer access between the distinct devices (xGMI copies of the exchanges)
        for (lsp_ctx* a : grp->ctxs)
            for (lsp_ctx* b : grp->ctxs)
                if (a->device != b->device) {
                    LSP_HIP(hipSetDevice(a->device));
                    int ok = 0;
                    LSP_HIP(hipDeviceCanAccessPeer(&ok, a->device, b->device));
                    if (ok) {
                        hipError_t e = hipDeviceEnablePeerAccess(b->device, 0);
                        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) LSP_HIP(e);
                        (void)hipGetLastError();
                    }
                }
        *out = grp;
    });
}

int lsp_group_destroy(lsp_group* grp) {
    delete grp;
    return LSP_OK;
}

int lsp_prove_group(lsp_group* grp, const lsp_fr* const* traces, size_t h, size_t w, const int32_t* air,
                    size_t air_len, const lsp_fr* pubv, size_t npub, int mem, lsp_proof** out) {
    lsp_ctx* c0 = grp && !grp->ctxs.empty() ? grp->ctxs[0] : nullptr;
    return guarded(c0, [&] {
        LSP_REQUIRE(grp && traces && out && pubv, LSP_E_ARG, "bad prove_group arguments");
        const int G = (int)grp->ctxs.size();
        const Air A = Air::parse(air, air_len);
        LSP_REQUIRE(A.prep_width == 0, LSP_E_ARG,
                    "the AIR reads preprocessed columns: the group prove has no preprocessed matrix");
        const std::vector<Fr> pub = to_frs(pubv, npub);
        ThreadGroup tg(G);
        for (int r = 0; r < G; ++r) tg.device[r] = grp->ctxs[r]->device;
        std::vector<lsp_proof*> res(G, nullptr);
        std::vector<int> code(G, LSP_OK);
        std::vector<std::string> msg(G);
        std::vector<std::thread> th;
        for (int r = 0; r < G; ++r) {
            th.emplace_back([&, r] {
                lsp_ctx* ctx = grp->ctxs[r];
                try {
                    std::lock_guard<std::mutex> lk(ctx->mu);
                    need_gpu(ctx);
                    const Fr* din = dev_in(ctx, traces[r], h * w, mem, "trace_in");
                    ThreadComm comm(&tg, r);
                    res[r] = prove_shard(ctx, comm, din, h, w, A, pub.data(), npub);
                } catch (const LspError& e) {
                    code[r] = e.code;
                    msg[r] = e.what();
                    tg.abort();
                } catch (const std::exception& e) {
                    code[r] = LSP_E_STATE;
                    msg[r] = e.what();
                    tg.abort();
                }
            });
        }
        for (auto& t : th) t.join();
        int bad = -1;
        for (int r = 0; r < G && bad < 0; ++r)  // report the first rank that failed on its own
            if (code[r] != LSP_OK && msg[r].find("another rank") == std::string::npos) bad = r;
        for (int r = 0; r < G && bad < 0; ++r)
            if (code[r] != LSP_OK) bad = r;
        if (bad < 0) {
            const std::vector<uint8_t> ref = serialize(*res[0]);
            for (int r = 1; r < G; ++r)
                if (serialize(*res[r]) != ref) {
                    bad = r;
                    code[r] = LSP_E_STATE;
                    msg[r] = "ranks disagree on the proof";
                }
        }
        for (int r = (bad < 0 ? 1 : 0); r < G; ++r) delete res[r];
        if (bad >= 0) throw LspError(code[bad], "rank " + std::to_string(bad) + ": " + msg[bad]);
        *out = res[0];
    });
}

int lsp_ctx_attach_comm_ops(lsp_ctx* ctx, const lsp_comm_ops* ops) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && ops && ops->allgather && ops->bcast, LSP_E_ARG, "bad communicator");
        LSP_REQUIRE(ops->size >= 1 && ops->rank >= 0 && ops->rank < ops->size, LSP_E_ARG, "bad rank / size");
        std::lock_guard<std::mutex> g(ctx->mu);
        delete ctx->comm;
        ctx->comm = make_callback_comm(*ops);
    });
}

int lsp_ctx_attach_loopback(lsp_ctx* ctx, int rank, int size) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && size >= 1 && rank >= 0 && rank < size, LSP_E_ARG, "bad rank / size");
        std::lock_guard<std::mutex> g(ctx->mu);
        delete ctx->comm;
        ctx->comm = new LoopbackComm(rank, size);
    });
}

int lsp_ctx_set_phase_timing(lsp_ctx* ctx, int on, const char* const* only, size_t n_only) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && (n_only == 0 || only), LSP_E_ARG, "null argument");
        std::vector<std::string> names;
        for (size_t i = 0; i < n_only; ++i) {
            LSP_REQUIRE(only[i], LSP_E_ARG, "null phase name");
            names.emplace_back(only[i]);
        }
        std::lock_guard<std::mutex> g(ctx->mu);
        ctx->phase_timing = on != 0;
        ctx->phase_only = std::move(names);
    });
}

int lsp_ctx_mem_stats(lsp_ctx* ctx, size_t* pool_bytes, size_t* device_used, size_t* device_total) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && pool_bytes && device_used && device_total, LSP_E_ARG, "null argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        size_t pool = 0;
        for (auto& kv : ctx->pool) pool += kv.second.cap;
        *pool_bytes = pool;
        size_t fr = 0, tot = 0;
        LSP_HIP(hipMemGetInfo(&fr, &tot));
        *device_used = tot - fr;
        *device_total = tot;
    });
}

int lsp_comm_rccl_unique_id(uint8_t id[128]) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(id, LSP_E_ARG, "null id");
        rccl_unique_id(id);
    });
}

int lsp_ctx_attach_rccl(lsp_ctx* ctx, const uint8_t id[128], int rank, int size) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && id && size >= 1 && rank >= 0 && rank < size, LSP_E_ARG, "bad RCCL attach arguments");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        delete ctx->comm;
        ctx->comm = nullptr;
        ctx->comm = make_rccl_comm(id, rank, size);
    });
}

int lsp_comm_selftest(lsp_ctx* ctx) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx, LSP_E_ARG, "null ctx");
        std::lock_guard<std::mutex> g(ctx->mu);
        LSP_REQUIRE(ctx->comm, LSP_E_STATE, "no communicator attached");
        need_gpu(ctx);
        Comm& c = *ctx->comm;
        const size_t n = 1000;  // words per rank, not a multiple of anything in particular
        std::vector<uint32_t> mine(n), got(n * (size_t)c.size);
        for (size_t i = 0; i < n; ++i) mine[i] = (uint32_t)(c.rank + 1) * 2654435761u + (uint32_t)i;
        uint32_t* s = (uint32_t*)ctx->buf("selftest_s", n * 4);
        uint32_t* r = (uint32_t*)ctx->buf("selftest_r", n * 4 * (size_t)c.size);
        LSP_HIP(hipMemcpyAsync(s, mine.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
        c.allgather(ctx, s, r, n * 4);
        LSP_HIP(hipMemcpyAsync(got.data(), r, got.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        LSP_HIP(hipStreamSynchronize(ctx->stream));
        for (int k = 0; k < c.size; ++k)
            for (size_t i = 0; i < n; ++i)
                LSP_REQUIRE(got[k * n + i] == (uint32_t)(k + 1) * 2654435761u + (uint32_t)i, LSP_E_STATE,
                            "communicator allgather returned wrong data");
        c.bcast(ctx, s, n * 4, 0);
        LSP_HIP(hipMemcpyAsync(got.data(), s, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        LSP_HIP(hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < n; ++i)
            LSP_REQUIRE(got[i] == 2654435761u + (uint32_t)i, LSP_E_STATE, "communicator bcast returned wrong data");
        calibrate_exchange(ctx, c);  // what the sharded proofs' inverse-NTT exchange is chosen on
    });
}

int lsp_comm_exchange_plan(lsp_ctx* ctx, size_t h, size_t w, size_t q, double* allgather_gbs, double* intt_gelem_s,
                           size_t* probe_bytes, int* split, double* allgather_ms, double* redundant_ms) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && split, LSP_E_ARG, "null argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        LSP_REQUIRE(ctx->comm, LSP_E_STATE, "no communicator attached");
        const Comm& c = *ctx->comm;
        LSP_REQUIRE(q == 0 || (q & (q - 1)) == 0, LSP_E_ARG, "q must be 0 or a power of two");
        const ExchangePlan p = exchange_plan(c, h, w, q, ctx->log_blowup);
        if (allgather_gbs) *allgather_gbs = c.ag_gbs;
        if (intt_gelem_s) *intt_gelem_s = c.intt_gelem_s;
        if (probe_bytes) *probe_bytes = c.ag_probe_bytes;
        *split = p.split ? 1 : 0;
        if (allgather_ms) *allgather_ms = p.allgather_ms;
        if (redundant_ms) *redundant_ms = p.redundant_ms;
    });
}

int lsp_comm_calibration(lsp_ctx* ctx, double* per_rank, size_t cap, size_t* n) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && n, LSP_E_ARG, "null argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        LSP_REQUIRE(ctx->comm, LSP_E_STATE, "no communicator attached");
        const std::vector<double>& raw = ctx->comm->calib_raw;
        *n = raw.size();
        if (per_rank && cap >= raw.size()) std::copy(raw.begin(), raw.end(), per_rank);
    });
}

int lsp_comm_quotient_exchange(lsp_ctx* ctx, size_t h, size_t q, size_t* bcasts, size_t* bytes_each,
                               double* model_ms) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx, LSP_E_ARG, "null ctx");
        std::lock_guard<std::mutex> g(ctx->mu);
        LSP_REQUIRE(ctx->comm, LSP_E_STATE, "no communicator attached");
        LSP_REQUIRE(q == 0 || (q & (q - 1)) == 0, LSP_E_ARG, "q must be 0 or a power of two");
        LSP_REQUIRE(h >= 2 && (h & (h - 1)) == 0, LSP_E_ARG, "h must be a power of two >= 2");
        const QuotientExchange x = quotient_exchange(*ctx->comm, h, q, ctx->log_blowup);
        if (bcasts) *bcasts = x.bcasts;
        if (bytes_each) *bytes_each = x.bytes_each;
        if (model_ms) *model_ms = x.model_ms;
    });
}

int lsp_ctx_host_threads(lsp_ctx* ctx, int* n) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && n, LSP_E_ARG, "null argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        *n = (int)ctx->host_pool().size();
    });
}

int lsp_comm_info(lsp_ctx* ctx, int* rank, int* size) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && rank && size, LSP_E_ARG, "null argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        LSP_REQUIRE(ctx->comm, LSP_E_STATE, "no communicator attached");
        *rank = ctx->comm->rank;
        *size = ctx->comm->size;
    });
}

int lsp_comm_log(lsp_ctx* ctx, char* ops, size_t* bytes, int* roots, double* ms, const char** tags, size_t cap,
                 size_t* n, double* init_ms) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && n, LSP_E_ARG, "null argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        LSP_REQUIRE(ctx->comm, LSP_E_STATE, "no communicator attached");
        need_gpu(ctx);
        Comm& c = *ctx->comm;
        c.resolve_log();
        *n = c.log.size();
        if (init_ms) *init_ms = c.init_ms;
        for (size_t i = 0; i < c.log.size() && i < cap; ++i) {
            const CommRec& r = c.log[i];
            if (ops) ops[i] = r.op;
            if (bytes) bytes[i] = r.bytes;
            if (roots) roots[i] = r.root;
            if (ms) ms[i] = r.ms;
            if (tags) tags[i] = r.tag.c_str();
        }
    });
}

int lsp_ctx_detach_comm(lsp_ctx* ctx) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx, LSP_E_ARG, "null ctx");
        std::lock_guard<std::mutex> g(ctx->mu);
        delete ctx->comm;
        ctx->comm = nullptr;
    });
}

int lsp_prove_sharded(lsp_ctx* ctx, const lsp_fr* trace, size_t h, size_t w, const int32_t* air, size_t air_len,
                      const lsp_fr* pubv, size_t npub, int mem, lsp_proof** out) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && out && pubv, LSP_E_ARG, "bad prove arguments");
        std::lock_guard<std::mutex> g(ctx->mu);
        LSP_REQUIRE(ctx->comm, LSP_E_STATE, "no communicator attached (lsp_ctx_attach_*)");
        need_gpu(ctx);
        const Air A = Air::parse(air, air_len);
        const std::vector<Fr> pub = to_frs(pubv, npub);
        const Fr* din = dev_in(ctx, trace, h * w, mem, "trace_in");
        *out = prove_shard(ctx, *ctx->comm, din, h, w, A, pub.data(), npub);
    });
}

int lsp_proof_serialize(const lsp_proof* p, uint8_t* buf, size_t cap, size_t* len) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(p && len, LSP_E_ARG, "null");
        std::lock_guard<std::mutex> g(p->cache_mu);
        if (p->wire.empty()) p->wire = serialize(*p);  // a size query and the copy serialize once
        const std::vector<uint8_t>& b = p->wire;
        *len = b.size();
        if (buf) {
            LSP_REQUIRE(!p->rehearsal, LSP_E_STATE,
                        "a rehearsal (loopback) proof is not a proof: only its size can be queried");
            LSP_REQUIRE(cap >= b.size(), LSP_E_ARG, "buffer too small");
            std::memcpy(buf, b.data(), b.size());
        }
    });
}

int lsp_proof_deserialize(const uint8_t* buf, size_t len, lsp_proof** out) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(buf && out, LSP_E_ARG, "null");
        *out = nullptr;
        *out = deserialize(buf, len);
    });
}

int lsp_proof_get_view(const lsp_proof* p, lsp_proof_view* view) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(p && view, LSP_E_ARG, "null");
        LSP_REQUIRE(!p->rehearsal, LSP_E_STATE, "a rehearsal (loopback) proof is not a proof");
        proof_view(*p, view);
    });
}

int lsp_proof_get_preprocessed_view(const lsp_proof* p, lsp_proof_preprocessed_view* view) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(p && view, LSP_E_ARG, "null argument");
        LSP_REQUIRE(!p->rehearsal, LSP_E_STATE, "a rehearsal proof holds fabricated data");
        proof_prep_view(*p, view);
    });
}

int lsp_proof_from_view(const lsp_proof_view* view, lsp_proof** out) {
    return guarded(nullptr, [&] {
        LSP_REQUIRE(view && out, LSP_E_ARG, "null");
        *out = nullptr;
        *out = proof_from_view(*view);
    });
}

int lsp_proof_free(lsp_proof* p) {
    proof_release(p);  // its wire bytes and query records are reused by the next proof
    return LSP_OK;
}

int lsp_verify(const lsp_ctx* ctx, const int32_t* air, size_t air_len, const lsp_fr* pubv, size_t npub,
               const uint8_t* proof, size_t len) {
    int rc = LSP_OK;
    int g = guarded(nullptr, [&] {
        LSP_REQUIRE(ctx && pubv && proof, LSP_E_ARG, "bad verify arguments");
        const Air A = Air::parse(air, air_len);
        LSP_REQUIRE(A.prep_width == 0, LSP_E_ARG,
                    "the AIR reads preprocessed columns: this call has no preprocessed commitment");
        const std::vector<Fr> pub = to_frs(pubv, npub);
        const int v = verify_host(ctx, A, pub.data(), npub, proof, len);
        if (v != 0) {
            g_err = "proof rejected at check " + std::to_string(v);
            rc = LSP_E_VERIFY;
        }
    });
    return g != LSP_OK ? g : rc;
}

int lsp_verify_preprocessed(const lsp_ctx* ctx, const int32_t* air, size_t air_len, const lsp_fr* pubv, size_t npub,
                            const lsp_fr* prep_commit, uint32_t prep_width, const uint8_t* proof, size_t len) {
    int rc = LSP_OK;
    int g = guarded(nullptr, [&] {
        LSP_REQUIRE(ctx && pubv && proof && prep_commit, LSP_E_ARG, "bad verify arguments");
        LSP_REQUIRE(prep_width >= 1 && prep_width <= (1u << 20), LSP_E_ARG, "preprocessed width outside [1, 2^20]");
        const Air A = Air::parse(air, air_len);
        LSP_REQUIRE(A.prep_width <= prep_width, LSP_E_ARG,
                    "the AIR reads " + std::to_string(A.prep_width) + " preprocessed columns of " +
                        std::to_string(prep_width));
        const std::vector<Fr> pub = to_frs(pubv, npub);
        const Fr root = to_fr(*prep_commit);
        const int v = verify_host(ctx, A, pub.data(), npub, proof, len, &root, prep_width);
        if (v != 0) {
            g_err = "proof rejected at check " + std::to_string(v);
            rc = LSP_E_VERIFY;
        }
    });
    return g != LSP_OK ? g : rc;
}

int lsp_last_timings(const lsp_ctx* ctx, double* ms, const char** names, size_t cap, size_t* n) {
    if (!ctx || !n) return LSP_E_ARG;
    // resolve_timings writes the context's timing state, which lsp_prove writes
    // too: the context's mutex serialises them (a Rust Ctx is Sync)
    lsp_ctx* c = const_cast<lsp_ctx*>(ctx);
    std::lock_guard<std::mutex> g(c->mu);
    try {
        lsp::resolve_timings(c);  // the events are the context's own
    } catch (...) {
        return LSP_E_HIP;
    }
    *n = ctx->timings.size();
    for (size_t i = 0; i < ctx->timings.size() && i < cap; ++i) {
        if (ms) ms[i] = ctx->timings[i].second;
        if (names) names[i] = ctx->timings[i].first.c_str();
    }
    return LSP_OK;
}

int lsp_last_spans(const lsp_ctx* ctx, const char** lines, size_t cap, size_t* n) {
    if (!ctx || !n) return LSP_E_ARG;
    std::lock_guard<std::mutex> g(const_cast<lsp_ctx*>(ctx)->mu);  // spans are rewritten by lsp_prove
    *n = ctx->spans.size();
    for (size_t i = 0; i < ctx->spans.size() && i < cap; ++i)
        if (lines) lines[i] = ctx->spans[i].c_str();
    return LSP_OK;
}

int lsp_calibrate_fr_mul(lsp_ctx* ctx, double* gmul_per_s) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && gmul_per_s, LSP_E_ARG, "null");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        const size_t nth = 256 * 256 * 16;  // 16 blocks of 256 lanes per CU
        const uint32_t iters = 256;
        Fr* out = ctx->fbuf("calib", nth);
        LSP_HIP(launch_calib_mul(out, nth, 8, ctx->stream));  // warm
        StreamTimer timer;
        const float ms = timer.ms(ctx->stream, [&] { LSP_HIP(launch_calib_mul(out, nth, iters, ctx->stream)); });
        *gmul_per_s = (double)nth * iters * 4 / (ms * 1e-3) / 1e9;
    });
}

int lsp_calibrate_poseidon2(lsp_ctx* ctx, double* mperm_per_s) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && mperm_per_s, LSP_E_ARG, "null");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        *mperm_per_s = calibrate_poseidon2(ctx);
    });
}

int lsp_calibrate_intt(lsp_ctx* ctx, uint32_t log_h, size_t w, double* gelem_per_s) {
    return guarded(ctx, [&] {
        LSP_REQUIRE(ctx && gelem_per_s, LSP_E_ARG, "null argument");
        LSP_REQUIRE(log_h >= 1 && log_h <= 26 && w >= 1 && w <= 1024 && (w << log_h) <= ((size_t)1 << 28), LSP_E_ARG,
                    "bad inverse-NTT probe shape (at most 2^28 elements)");
        std::lock_guard<std::mutex> g(ctx->mu);
        need_gpu(ctx);
        *gelem_per_s = calibrate_intt(ctx, log_h, w, 5, nullptr);
        ctx->release("calib_intt_");
    });
}

}  // extern "C"
