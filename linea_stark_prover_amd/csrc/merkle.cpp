// The Merkle commit: wide levels on the GPU, the tree top on the host pool.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "comm.hpp"
#include "host.hpp"
#include "host_slice.hpp"
#include "prove_internal.hpp"

namespace lsp {

// MerkleTreeMmcs::commit of `m` into `layers` (2*height - 1 digests, leaves
// first).  Wide levels run on the GPU; once a layer has at most
// host_tree_top digests the remaining levels are a few dozen permutations on
// the critical path, and the host (a ~30 ns multiply against ~350 ns for one
// wave's multiply chain) finishes them with a small thread pool.  Trees of
// at most host_tree_top single-matrix rows are hashed on the host entirely.
// The host layers go back to the device (openings gather from device memory)
// from a pinned staging buffer, without waiting: the next use of the buffer
// comes after a later synchronisation of the same stream.
// Under the leaves and wide levels of a big tree the pool is not idle either:
// it hashes the tree's last 1/32 .. 1/128 -- the host slice, below.
// LSP_TIME_TOPS=1: host-side timing of the tree tops (diagnostic), printed at exit
struct TopTimes {
    bool on = std::getenv("LSP_TIME_TOPS") != nullptr;
    double sync_us = 0, levels_us = 0, first_us = 0;
    size_t n = 0;
    // per tree (the last ones are printed): host time since the previous tree's
    // return, launch issue, sleep until ev_near, spin until ev_top, host levels
    // (near includes the host slice, given apart)
    struct Rec { size_t height; double since_prev, launch, near, spin, levels, slice; };
    std::vector<Rec> recs;
    host_clock::time_point last_exit{};
    ~TopTimes() {
        if (on && n) {
            std::fprintf(stderr, "[tree tops] %zu trees: wait-for-GPU %.1f us, host levels %.1f us (first level %.1f us) per tree\n",
                         n, sync_us / n, levels_us / n, first_us / n);
            const size_t k = recs.size() < 16 ? 0 : recs.size() - 16;
            for (size_t i = k; i < recs.size(); ++i)
                std::fprintf(stderr, "[tree] height %9zu  since-prev %7.1f  launch %6.1f  near %8.1f  spin %7.1f  levels %6.1f  host slice %8.1f us\n",
                             recs[i].height, recs[i].since_prev, recs[i].launch, recs[i].near, recs[i].spin, recs[i].levels, recs[i].slice);
        }
    }
};
static TopTimes g_top_times;
bool time_tops() { return g_top_times.on; }

// Proofs running at once in this process (several contexts in flight, or the
// ranks of an in-process group).  A lone proof hands its trees to the host
// pool from host_tree_top digests; concurrent proofs share the host's cores,
// so there the host takes over only from 256 digests (bench, same box:
// 1024 vs 256 = 67.6 vs 68.3 ms alone, 62.3 vs 60.0 ms per proof with three in flight).
static std::atomic<int> g_active_proofs{0};
ActiveProof::ActiveProof() { g_active_proofs.fetch_add(1, std::memory_order_relaxed); }
ActiveProof::~ActiveProof() { g_active_proofs.fetch_sub(1, std::memory_order_relaxed); }
constexpr size_t SHARED_HOST_TREE_TOP = 256;

// out[i] = compress(in[2i], in[2i+1]) for i < half on the host pool
static void host_compress_level(lsp_ctx* ctx, const Fr* in, Fr* out, size_t half) {
    HostPool& pool = ctx->host_pool();
    if (half <= pool.size())  // one permutation per thread: the scalar path's latency is lower
        pool.parallel_for(half, [&](size_t i) { out[i] = ctx->p2.compress(in[2 * i], in[2 * i + 1]); });
    else {  // 8 or 16 at a time (AVX-512 IFMA when the CPU has it)
        const size_t blk = half >= 16 * pool.size() ? 16 : 8;
        pool.parallel_for((half + blk - 1) / blk, [&](size_t b) {
            ctx->p2.compress_range(in, out, blk * b, std::min(half, blk * b + blk));
        });
    }
}

// The levels above `first` digests host[0, first): each level is appended
// after the one below it; returns the end of the layers (the root is
// host[end - 1]).  *t_first (if given) is set after the first level.
// pairs (optional): the `first` digests are made first, as the 2-element
// leaves compress(pairs[2i], pairs[2i+1]) of a FRI round (A4/A5), inside the
// same tasks.
// The tree splits into P = (pool threads, a power of two) subtrees of
// first / P digests, one task each: a task hashes its leaves and every level
// of its subtree with no barrier in between (a parallel_for costs ~5 us, as
// much as an 8-lane IFMA batch, and the levels below 16 digests per thread
// used to take one each), and the log2 P levels above the subtree roots run on
// this thread.  Each task keeps >= 16 digests (fewer threads for small
// trees).  LSP_HOST_SUBTREE=0: level by level, one parallel_for each.
size_t host_levels(lsp_ctx* ctx, Fr* host, size_t first, host_clock::time_point* t_first, const Fr* pairs) {
    static const bool subtrees = [] {
        const char* e = std::getenv("LSP_HOST_SUBTREE");
        return !(e && *e == '0');
    }();
    HostPool& pool = ctx->host_pool();
    if (first <= 1) {
        if (pairs && first == 1) host[0] = ctx->p2.compress(pairs[0], pairs[1]);
        if (t_first) *t_first = std::chrono::steady_clock::now();
        return first;
    }
    // level j >= 0 holds first >> j digests at off[j]
    size_t off[64];
    uint32_t nl = 0;
    off[0] = 0;
    size_t end = first;
    for (size_t c = first / 2; c >= 1; c /= 2) {
        off[++nl] = end;
        end += c;
    }
    auto level_part = [&](uint32_t j, size_t i0, size_t cnt) {  // level j, digests [i0, i0 + cnt)
        if (cnt == 1)
            host[off[j] + i0] = ctx->p2.compress(host[off[j - 1] + 2 * i0], host[off[j - 1] + 2 * i0 + 1]);
        else
            ctx->p2.compress_range(host + off[j - 1], host + off[j], i0, i0 + cnt);
    };
    auto leaf_part = [&](size_t i0, size_t cnt) {
        if (cnt == 1)
            host[i0] = ctx->p2.compress(pairs[2 * i0], pairs[2 * i0 + 1]);
        else
            ctx->p2.compress_range(pairs, host, i0, i0 + cnt);
    };
    if (!subtrees) {
        if (pairs) host_compress_level(ctx, pairs, host, first);
        for (uint32_t j = 1; j <= nl; ++j) {
            host_compress_level(ctx, host + off[j - 1], host + off[j], first >> j);
            if (j == 1 && t_first) *t_first = std::chrono::steady_clock::now();
        }
        return end;
    }
    size_t P = 1;
    while (2 * P <= pool.size() && first / (2 * P) >= 16) P *= 2;
    const size_t per = first / P;
    const uint32_t sl = log2_exact(per);  // levels inside a task
    auto task = [&](size_t p) {
        if (pairs) leaf_part(p * per, per);
        for (uint32_t j = 1; j <= sl; ++j) level_part(j, p * (per >> j), per >> j);
    };
    if (P > 1)
        pool.parallel_for(P, task);
    else
        task(0);
    if (t_first) *t_first = std::chrono::steady_clock::now();
    for (uint32_t j = sl + 1; j <= nl; ++j) level_part(j, 0, first >> j);  // above the task roots
    return end;
}

// the pinned buffer of a tree's host layers: one per tree while uploads are
// deferred (each must stay intact until flush_top_uploads), else one shared
static std::string top_buf_name(lsp_ctx* ctx) {
    return ctx->defer_top_uploads ? "merkle_top" + std::to_string(ctx->top_uploads.size()) : std::string("merkle_top");
}

// issue the deferred tree-top uploads on the context's stream, behind the host
// slices' layers (slice_hash sent those up on the side stream)
void flush_top_uploads(lsp_ctx* ctx) {
    if (ctx->slice_uploads_pending) {
        LSP_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_slice_up, 0));
        ctx->slice_uploads_pending = false;
    }
    for (const auto& u : ctx->top_uploads)
        LSP_HIP(hipMemcpyAsync(u.dst, u.src, u.bytes, hipMemcpyHostToDevice, ctx->stream));
    ctx->top_uploads.clear();
}

DeferTopUploads::DeferTopUploads(lsp_ctx* c) : ctx(c) {
    ctx->top_uploads.clear();
    ctx->defer_top_uploads = std::getenv("LSP_NO_DEFER_TOPS") == nullptr;
}
DeferTopUploads::~DeferTopUploads() {
    ctx->defer_top_uploads = false;
    ctx->slice_uploads_pending = false;
    ctx->top_uploads.clear();
}

// LSP_TOP_ZEROCOPY=0: the last GPU level goes to HBM and a copy brings it to the host
static bool zerocopy_top() {
    static const bool on = [] {
        const char* e = std::getenv("LSP_TOP_ZEROCOPY");
        return !(e && *e == '0');
    }();
    return on;
}

// levels above this many digests fill the chip; the ones below run one wave per
// SIMD or fewer (per-level rates)
constexpr size_t WIDE_LEVEL_STOP = (size_t)1 << 16;

// The host pool starts spinning when a tree's GPU levels are down to this many
// digests (ev_warm), not only for the last two levels (ev_near): after a GPU
// phase of milliseconds the pool's cores, asleep meanwhile, ran the tree top's
// first parallel_for 20-75 us slower than cores kept busy, unless they had been
// spinning for about a millisecond (LSP_TIME_TOPS per tree: 2^16 and 2^18 still
// left the 4M-leaf trees slow, 2^20 -- 1.5-2.7 ms ahead -- made every tree top
// as fast as the narrow trees').  Read per call; LSP_TOP_WARM=0: off.  By
// default only while this proof has the host to itself: with several proofs in
// flight in the process or several ranks on the host (LOCAL_WORLD_SIZE > 1) the
// pools' spinning competed with the other proofs' host work (eight ranks
// sharing one GPU and 16 CPUs: 19 % slower), for nothing the GPU waits on.
static bool shared_host() {  // several ranks on this host
    static const bool v = [] {
        const char* e = std::getenv("LOCAL_WORLD_SIZE");
        return e && std::strtol(e, nullptr, 10) > 1;
    }();
    return v;
}
static size_t top_warm_nodes(const lsp_ctx* ctx) {
    if (const char* e = std::getenv("LSP_TOP_WARM")) return (size_t)std::strtoull(e, nullptr, 10);
    if (shared_host() || ctx->comm || g_active_proofs.load(std::memory_order_relaxed) > 1) return 0;
    return (size_t)1 << 20;
}
constexpr unsigned TOP_WARM_SPIN_US = 5000;  // bound on the pool's spin after ev_warm

// busy-wait for an event that is microseconds away (a sleeping wait wakes up late)
static void spin_until(hipEvent_t ev) {
    hipError_t q;
    while ((q = hipEventQuery(ev)) == hipErrorNotReady) {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    LSP_HIP(q);
}

size_t host_tree_top(const lsp_ctx* ctx) {
    size_t top = ctx->host_tree_top;
    if (g_active_proofs.load(std::memory_order_relaxed) > 1) top = std::min(top, SHARED_HOST_TREE_TOP);
    return env_size("LSP_HOST_TREE_TOP", top);
}

// ---- the host slice of a big tree (host_slice.hpp)
double calibrate_poseidon2(lsp_ctx* ctx) {
    // the peak: best of several grid sizes (2..32 blocks of 256 lanes per CU)
    const uint32_t iters = 4;
    Fr* out = ctx->fbuf("calib", (size_t)256 * 256 * 32);
    LSP_HIP(launch_calib_perm(out, (size_t)256 * 256 * 4, 1, ctx->rc29_dev, ctx->p2.L, ctx->stream));  // warm
    StreamTimer timer;
    double best = 0;
    for (size_t per_cu : {2, 4, 8, 16, 32}) {
        const size_t nth = (size_t)256 * 256 * per_cu;
        const float ms = timer.ms(ctx->stream, [&] {
            LSP_HIP(launch_calib_perm(out, nth, iters, ctx->rc29_dev, ctx->p2.L, ctx->stream));
        });
        best = std::max(best, (double)nth * iters / (ms * 1e-3) / 1e6);
    }
    return best;
}

// The whole pool's rate at a slice's work, permutations/s: the best of three
// timed jobs (the one before them wakes the pool) whose tasks are slice_hash's
// -- 256 rows of 8 columns through the row sponge, then their subtree.  (Bare
// compressions, 16 lanes in lockstep, run a third faster than a slice does:
// 25.6 against 19-20 M/s on the 16 threads of the bench's box.)
static double host_pool_perm_rate(lsp_ctx* ctx) {
    HostPool& pool = ctx->host_pool();
    const size_t per = 256, w = 8, tasks = 8 * (size_t)pool.size();
    std::vector<Fr> rows(per * w * tasks), lay(2 * per * tasks);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = fr_from_u64(i + 1);
    double best = 0;
    for (int rep = 0; rep < 4; ++rep) {
        const auto t0 = host_clock::now();
        pool.parallel_for(tasks, [&](size_t t) {
            Fr* l = lay.data() + 2 * per * t;  // this task's levels, one after the other
            ctx->p2.hash_range(rows.data() + per * w * t, w, l, 0, per);
            for (size_t n = per / 2; n >= 1; l += 2 * n, n /= 2) ctx->p2.compress_range(l, l + 2 * n, 0, n);
        });
        const double s = us(t0, host_clock::now()) * 1e-6;
        if (rep) best = std::max(best, (double)(tasks * (per * w / 2 + per - 1)) / s);
    }
    return best;
}

// The slice of a tree of `height` leaves whose host top starts from `top`
// digests.  LSP_HOST_SLICE, read per call: 0 = off, k = log_frac k whatever the
// size, the rates and the sharing.  Otherwise only inside a lone proof (not in
// the fine-grained C API, whose caller may be using the host), with the host to
// itself as for the warm-up above, and as the two rates -- measured at the
// context's first big tree -- allow.  The halves meet in the coherent buffer the
// last GPU level writes, so there is no slice without one.
static HostSlice plan_slice(lsp_ctx* ctx, const MatList& m, size_t height, size_t top) {
    HostSliceIn in;
    const char* e = std::getenv("LSP_HOST_SLICE");
    in.forced = e ? std::max(-1, (int)std::strtol(e, nullptr, 10)) : -1;
    if (in.forced == 0 || !zerocopy_top() || top == 0 || height < 2 * top) return {};
    in.leaves = height;
    in.join = top;
    size_t w = 0;
    for (uint32_t k = 0; k < m.n; ++k) w += m.width[k];
    in.perms_per_leaf = (w + 1) / 2;
    in.shared = shared_host() || ctx->comm || g_active_proofs.load(std::memory_order_relaxed) != 1;
    if (in.forced < 0) {
        if (in.shared || height < HOST_SLICE_MIN_LEAVES) return {};
        if (!(ctx->slice_host_perm_s > 0)) {
            ctx->slice_gpu_perm_s = calibrate_poseidon2(ctx) * 1e6;
            ctx->slice_host_perm_s = host_pool_perm_rate(ctx);
            if (g_top_times.on)
                std::fprintf(stderr, "[host slice] rates: host pool %.1f, GPU %.1f M permutations/s\n",
                             ctx->slice_host_perm_s * 1e-6, ctx->slice_gpu_perm_s * 1e-6);
        }
        in.host_perm_s = ctx->slice_host_perm_s;
        in.gpu_perm_s = ctx->slice_gpu_perm_s;
    }
    return plan_host_slice(in);
}

// A slice's pinned buffer: its layers below the join layer (level j, of S >> j
// digests, at TreeLayout{S}.offset(j)), then its rows, matrix after matrix.
struct SliceBuf {
    HostSlice hs;
    size_t S = 0, J = 0, W = 0;  // leaves, digests of the join layer, row width over all matrices
    uint32_t nj = 0;             // levels from the leaves to the join layer
    Fr* buf = nullptr;
    Fr* rows() const { return buf + TreeLayout{S}.offset(nj); }
};

hipStream_t slice_stream_begin(lsp_ctx* ctx) {
    if (!ctx->ev_slice) {
        LSP_HIP(hipEventCreateWithFlags(&ctx->ev_slice_in, hipEventDisableTiming));
        LSP_HIP(hipEventCreateWithFlags(&ctx->ev_slice, hipEventDisableTiming));
        LSP_HIP(hipEventCreateWithFlags(&ctx->ev_slice_up, hipEventDisableTiming));
    }
    hipStream_t sd = ctx->side();
    LSP_HIP(hipEventRecord(ctx->ev_slice_in, ctx->stream));
    LSP_HIP(hipStreamWaitEvent(sd, ctx->ev_slice_in, 0));
    return sd;
}
void slice_stream_end(lsp_ctx* ctx) { LSP_HIP(hipEventRecord(ctx->ev_slice, ctx->side())); }

void host_hash_rows(const P2Host& p2, const Fr* const* rows, const size_t* width, size_t n, Fr* out, size_t i0,
                    size_t i1) {
    if (n == 1) {
        p2.hash_range(rows[0], width[0], out, i0, i1);
        return;
    }
    size_t W = 0;
    for (size_t k = 0; k < n; ++k) W += width[k];
    std::vector<Fr> cat((i1 - i0) * W);
    for (size_t k = 0, c0 = 0; k < n; c0 += width[k++])
        for (size_t i = i0; i < i1; ++i)
            std::copy(rows[k] + i * width[k], rows[k] + (i + 1) * width[k], &cat[(i - i0) * W + c0]);
    p2.hash_range(cat.data(), W, out + i0, 0, i1 - i0);
}

// the slice's rows into pinned memory, on the side stream, from the moment the
// main stream's work so far -- what makes the tree's input -- is done
static SliceBuf slice_download(lsp_ctx* ctx, const MatList& m, size_t height, size_t top, HostSlice hs,
                               const std::string& name) {
    SliceBuf b;
    b.hs = hs;
    b.S = hs.slice(height);
    b.J = hs.slice(top);
    b.nj = log2_exact(b.S / b.J);
    for (uint32_t k = 0; k < m.n; ++k) b.W += m.width[k];
    b.buf = (Fr*)ctx->hbuf(name, (TreeLayout{b.S}.offset(b.nj) + b.S * b.W) * sizeof(Fr));
    hipStream_t sd = slice_stream_begin(ctx);
    Fr* dst = b.rows();
    for (uint32_t k = 0; k < m.n; ++k) {
        const size_t w = m.width[k];
        LSP_HIP(hipMemcpyAsync(dst, m.ptr[k] + (height - b.S) * w, b.S * w * sizeof(Fr), hipMemcpyDeviceToHost, sd));
        dst += b.S * w;
    }
    slice_stream_end(ctx);
    return b;
}

// The slice on the host pool, once its rows have arrived: the leaves with the
// host row sponge and every level up to the join layer, whose J digests go to
// `join` (beside the GPU's, in the tree top's buffer).  Tasks of up to 256
// leaves hash their rows and their own subtree with no barrier per level; a
// second job finishes the J subtrees above the task roots.  The layers below
// the join go up into the suffix of each device layer like the tree tops.
static void slice_hash(lsp_ctx* ctx, const MatList& m, size_t height, const SliceBuf& b, Fr* join, Fr* layers) {
    LSP_HIP(hipEventSynchronize(ctx->ev_slice));
    HostPool& pool = ctx->host_pool();
    const TreeLayout sl{b.S};
    auto level = [&](uint32_t j) { return j == b.nj ? join : b.buf + sl.offset(j); };
    const size_t per = std::min<size_t>(b.S / b.J, 256);
    const uint32_t lp = log2_exact(per);
    const Fr* rows[8];
    size_t width[8];
    for (uint32_t k = 0; k < m.n; ++k) {
        width[k] = m.width[k];
        rows[k] = k ? rows[k - 1] + b.S * width[k - 1] : b.rows();
    }
    pool.parallel_for(b.S / per, [&](size_t t) {
        const size_t i0 = t * per;
        host_hash_rows(ctx->p2, rows, width, m.n, level(0), i0, i0 + per);
        for (uint32_t j = 1; j <= lp; ++j) ctx->p2.compress_range(level(j - 1), level(j), i0 >> j, (i0 + per) >> j);
    });
    if (lp < b.nj)
        pool.parallel_for(b.J, [&](size_t p) {
            for (uint32_t j = lp + 1; j <= b.nj; ++j) {
                const size_t c = (b.S >> j) / b.J;
                ctx->p2.compress_range(level(j - 1), level(j), p * c, (p + 1) * c);
            }
        });
    // Megabytes, not the tree top's kilobytes: queued for flush_top_uploads they
    // were 0.4 ms of copies ahead of a 2^19 proof's query phase.  While uploads
    // are deferred they go on the side stream at once, under the GPU's levels,
    // and flush_top_uploads makes the main stream wait for the last of them.
    const TreeLayout lay{height};
    hipStream_t up = ctx->defer_top_uploads ? ctx->side() : ctx->stream;
    for (uint32_t j = 0; j < b.nj; ++j)
        LSP_HIP(hipMemcpyAsync(layers + lay.offset(j) + b.hs.prefix(lay.len(j)), level(j), (b.S >> j) * sizeof(Fr),
                               hipMemcpyHostToDevice, up));
    if (ctx->defer_top_uploads) {
        LSP_HIP(hipEventRecord(ctx->ev_slice_up, up));
        ctx->slice_uploads_pending = true;
    }
}

Fr commit_device(lsp_ctx* ctx, const MatList& m, size_t height, Fr* layers, size_t top, const FoldSpec* fold,
                 const std::function<void(hipEvent_t)>* side) {
    hipStream_t st = ctx->stream;
    using clk = host_clock;
    const auto tt0 = clk::now();
    auto t_launched = tt0, t_near = tt0;
    HostPool& pool = ctx->host_pool();
    size_t off = 0, len = height;
    if (fold && height <= top && height > 1) {
        // a short vector: materialise the fold, then the host path below hashes it
        LSP_HIP(launch_fri_fold(*fold, 2 * height, st));
        fold = nullptr;
    }
    const bool leaves_on_host = height <= top && m.n == 1 && height > 1;
    bool gpu_level_on_host = false;  // the last GPU level was written into `host` directly
    Fr* host;  // host layers, starting at device offset `off` (pinned)
    const std::string tbuf = top_buf_name(ctx);  // of the tree's pinned buffers: "", "c" (coherent), "s" (slice)
    double slice_us = 0;
    if (leaves_on_host) {
        const size_t w = m.width[0];
        host = (Fr*)ctx->hbuf(tbuf, (TreeLayout{height}.size() + height * w) * sizeof(Fr));
        Fr* rows = host + TreeLayout{height}.size();
        LSP_HIP(hipMemcpyAsync(rows, m.ptr[0], height * w * sizeof(Fr), hipMemcpyDeviceToHost, st));
        if (side) {  // nothing left on the GPU for this tree
            LSP_HIP(hipEventRecord(ctx->ev_wide, st));
            (*side)(ctx->ev_wide);
        }
        LSP_HIP(hipStreamSynchronize(st));
        pool.parallel_for((height + 7) / 8, [&](size_t b) {
            ctx->p2.hash_range(rows, w, host, 8 * b, std::min(height, 8 * b + 8));
        });
    } else {
        // the host's part of the leaves and of every layer below `top` digests
        // (no slice: none).  A fused fold has none: its folded vector is the
        // next round's input, and only round 0 -- which folds nothing -- is big
        const HostSlice hs = fold ? HostSlice{} : plan_slice(ctx, m, height, top);
        SliceBuf sb;
        if (hs) sb = slice_download(ctx, m, height, top, hs, tbuf + "s");
        if (fold)
            LSP_HIP(launch_fold_hash(*fold, height, layers, ctx->rc29_dev, ctx->p2.L, st));
        else
            LSP_HIP(launch_hash_rows(m, hs.prefix(height), layers, ctx->rc29_dev, ctx->p2.L, st));
        if (top == 0) {
            LSP_HIP(launch_merkle_tree(layers, height, ctx->rc29_dev, ctx->p2.L, st));
            if (side) {
                LSP_HIP(hipEventRecord(ctx->ev_wide, st));
                (*side)(ctx->ev_wide);
            }
            return d2h_fr(ctx, layers + TreeLayout{height}.root());
        }
        if (!ctx->ev_near) {
            LSP_HIP(hipEventCreateWithFlags(&ctx->ev_near, hipEventDisableTiming));
            LSP_HIP(hipEventCreateWithFlags(&ctx->ev_top, hipEventDisableTiming));
            LSP_HIP(hipEventCreateWithFlags(&ctx->ev_warm, hipEventDisableTiming));
        }
        // the wide levels; the side work's / the host pool's event; the narrow ones
        // down to 4 top; an event; the last two (~100 us) and the download
        const size_t warm = top_warm_nodes(ctx);
        // stops (largest first) after which an event goes on the stream
        struct Stop {
            size_t nodes;
            hipEvent_t ev;
        } stops[2];
        int nstops = 0;
        if (warm) stops[nstops++] = {std::max(4 * top, warm), ctx->ev_warm};
        if (side) stops[nstops++] = {std::max(4 * top, WIDE_LEVEL_STOP), ctx->ev_wide};
        if (nstops == 2 && stops[1].nodes > stops[0].nodes) std::swap(stops[0], stops[1]);
        // the GPU levels so far end at layers + off1, in a level of len1 digests
        size_t off1 = 0, len1 = height;
        auto levels_to = [&](size_t stop, hipEvent_t ev = nullptr) {  // the levels down to `stop` digests
            size_t o = 0, l = len1;
            LSP_HIP(launch_merkle_levels(layers + off1, len1, stop, ctx->rc29_dev, ctx->p2.L, &o, &l, st, hs.log_frac));
            if (ev) LSP_HIP(hipEventRecord(ev, st));
            off1 += o;
            len1 = l;
        };
        for (int k = 0; k < nstops; ++k) levels_to(stops[k].nodes, stops[k].ev);
        levels_to(4 * top, ctx->ev_near);
        if (zerocopy_top()) levels_to(2 * top);
        if (zerocopy_top() && len1 > top) {
            // down to 2 top digests in HBM; the last GPU level writes its `top`
            // digests straight into the pinned host buffer (no copy kernel on the
            // critical path); the upload below takes them back to HBM
            off = off1;
            len = len1 / 2;
            // fine-grained (coherent) pinned memory: the kernel's stores bypass the
            // GPU caches, so they are in host memory when the kernel completes
            host = (Fr*)ctx->hbuf(tbuf + "c", TreeLayout{len}.size() * sizeof(Fr), hipHostMallocCoherent);
            LSP_HIP(launch_merkle_level(layers + off, host, hs.prefix(len), ctx->rc29_dev, ctx->p2.L, st));
            off += len1;
            gpu_level_on_host = true;
        } else {  // LSP_TOP_ZEROCOPY=0, or no GPU level left above `top` digests: copy them
            if (!zerocopy_top()) levels_to(top);
            off = off1;
            len = len1;
            LSP_REQUIRE(!hs, LSP_E_STATE, "a host slice without the coherent tree top");  // (plan_slice)
            host = (Fr*)ctx->hbuf(tbuf, TreeLayout{len}.size() * sizeof(Fr));
            LSP_HIP(hipMemcpyAsync(host, layers + off, len * sizeof(Fr), hipMemcpyDeviceToHost, st));
        }
        LSP_HIP(hipEventRecord(ctx->ev_top, st));
        if (side) (*side)(ctx->ev_wide);
        t_launched = clk::now();
        // sleep through the wide levels, then spin (with the pool awake) for the last ones
        resolve_timings(ctx);  // the previous proof's phase events, meanwhile
        if (hs) {
            // under the GPU's leaves and wide levels.  On this thread, one of the
            // pool's: it has nothing to do but wait; and ahead of the warm-up, which
            // needs the pool -- a slice that ends late finds the events below passed
            const auto ts0 = clk::now();
            slice_hash(ctx, m, height, sb, host + hs.prefix(len), layers);
            slice_us = us(ts0, clk::now());
        }
        if (warm) {
            LSP_HIP(hipEventSynchronize(ctx->ev_warm));
            pool.wake(TOP_WARM_SPIN_US);
            spin_until(ctx->ev_near);
            t_near = clk::now();
        } else {
            LSP_HIP(hipEventSynchronize(ctx->ev_near));
            t_near = clk::now();
            pool.wake();
        }
        spin_until(ctx->ev_top);
    }
    const auto tt1 = clk::now();
    auto tt2 = tt1;
    const size_t first = len;  // the part already on the device (unless hashed here)
    const size_t end = host_levels(ctx, host, first, &tt2);
    if (g_top_times.on) {
        const auto tt3 = clk::now();
        g_top_times.n++;
        g_top_times.sync_us += us(tt0, tt1);
        g_top_times.levels_us += us(tt1, tt3);
        g_top_times.first_us += us(tt1, tt2);
        g_top_times.recs.push_back({height, g_top_times.last_exit == clk::time_point{} ? 0.0 : us(g_top_times.last_exit, tt0),
                                    us(tt0, t_launched), us(t_launched, t_near), us(t_near, tt1), us(tt1, tt3), slice_us});
        g_top_times.last_exit = clk::now();
    }
    // digests that exist only on the host start here
    const size_t skip = leaves_on_host || gpu_level_on_host ? 0 : first;
    if (end > skip) {
        if (ctx->defer_top_uploads)
            ctx->top_uploads.push_back({layers + off + skip, host + skip, (end - skip) * sizeof(Fr)});
        else
            LSP_HIP(hipMemcpyAsync(layers + off + skip, host + skip, (end - skip) * sizeof(Fr), hipMemcpyHostToDevice, st));
    }
    return host[end - 1];
}

// Root of a Merkle tree whose 2^b bottom subtrees live on the 2^b ranks
// (rank r's subtree root = `local`, leaves r*S .. (r+1)*S - 1).  `top` gets
// the b + 1 host layers above the subtrees (top[0] = the rank roots).
Fr shard_root(lsp_ctx* ctx, Comm& comm, const Fr& local, std::vector<std::vector<Fr>>& top, const char* tag) {
    if (comm.size == 1) {
        top.assign(1, std::vector<Fr>(1, local));
        return local;
    }
    top.assign(1, comm.allgather_fr(ctx, &local, 1, tag));
    while (top.back().size() > 1) {
        const std::vector<Fr>& lo = top.back();
        std::vector<Fr> up(lo.size() / 2);
        for (size_t i = 0; i < up.size(); ++i) up[i] = ctx->p2.compress(lo[2 * i], lo[2 * i + 1]);
        top.push_back(std::move(up));
    }
    return top.back()[0];
}

}  // namespace lsp
