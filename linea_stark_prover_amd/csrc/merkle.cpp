// The Merkle commit: wide levels on the GPU, the tree top on the host pool.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "comm.hpp"
#include "host.hpp"
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
// LSP_TIME_TOPS=1: host-side timing of the tree tops (diagnostic), printed at exit
struct TopTimes {
    bool on = std::getenv("LSP_TIME_TOPS") != nullptr;
    double sync_us = 0, levels_us = 0, first_us = 0;
    size_t n = 0;
    // per tree (the last ones are printed): host time since the previous tree's
    // return, launch issue, sleep until ev_near, spin until ev_top, host levels
    struct Rec { size_t height; double since_prev, launch, near, spin, levels; };
    std::vector<Rec> recs;
    host_clock::time_point last_exit{};
    ~TopTimes() {
        if (on && n) {
            std::fprintf(stderr, "[tree tops] %zu trees: wait-for-GPU %.1f us, host levels %.1f us (first level %.1f us) per tree\n",
                         n, sync_us / n, levels_us / n, first_us / n);
            const size_t k = recs.size() < 16 ? 0 : recs.size() - 16;
            for (size_t i = k; i < recs.size(); ++i)
                std::fprintf(stderr, "[tree] height %9zu  since-prev %7.1f  launch %6.1f  near %8.1f  spin %7.1f  levels %6.1f us\n",
                             recs[i].height, recs[i].since_prev, recs[i].launch, recs[i].near, recs[i].spin, recs[i].levels);
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

// issue the deferred tree-top uploads on the context's stream
void flush_top_uploads(lsp_ctx* ctx) {
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
static size_t top_warm_nodes(const lsp_ctx* ctx) {
    if (const char* e = std::getenv("LSP_TOP_WARM")) return (size_t)std::strtoull(e, nullptr, 10);
    static const bool shared_host = [] {
        const char* e = std::getenv("LOCAL_WORLD_SIZE");
        return e && std::strtol(e, nullptr, 10) > 1;
    }();
    if (shared_host || ctx->comm || g_active_proofs.load(std::memory_order_relaxed) > 1) return 0;
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
    if (leaves_on_host) {
        const size_t w = m.width[0];
        host = (Fr*)ctx->hbuf(top_buf_name(ctx), (TreeLayout{height}.size() + height * w) * sizeof(Fr));
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
        if (fold)
            LSP_HIP(launch_fold_hash(*fold, height, layers, ctx->rc29_dev, ctx->p2.L, st));
        else
            LSP_HIP(launch_hash_rows(m, height, layers, ctx->rc29_dev, ctx->p2.L, st));
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
            LSP_HIP(launch_merkle_levels(layers + off1, len1, stop, ctx->rc29_dev, ctx->p2.L, &o, &l, st));
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
            host = (Fr*)ctx->hbuf(top_buf_name(ctx) + "c", TreeLayout{len}.size() * sizeof(Fr), hipHostMallocCoherent);
            LSP_HIP(launch_merkle_level(layers + off, host, len, ctx->rc29_dev, ctx->p2.L, st));
            off += len1;
            gpu_level_on_host = true;
        } else {  // LSP_TOP_ZEROCOPY=0, or no GPU level left above `top` digests: copy them
            if (!zerocopy_top()) levels_to(top);
            off = off1;
            len = len1;
            host = (Fr*)ctx->hbuf(top_buf_name(ctx), TreeLayout{len}.size() * sizeof(Fr));
            LSP_HIP(hipMemcpyAsync(host, layers + off, len * sizeof(Fr), hipMemcpyDeviceToHost, st));
        }
        LSP_HIP(hipEventRecord(ctx->ev_top, st));
        if (side) (*side)(ctx->ev_wide);
        t_launched = clk::now();
        // sleep through the wide levels, then spin (with the pool awake) for the last ones
        resolve_timings(ctx);  // the previous proof's phase events, meanwhile
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
                                    us(tt0, t_launched), us(t_launched, t_near), us(t_near, tt1), us(tt1, tt3)});
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
