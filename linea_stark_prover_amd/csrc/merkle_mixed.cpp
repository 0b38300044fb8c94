// MerkleTreeMmcs over matrices of unequal heights:
// the tallest matrices make the leaves, every class of shorter ones is hashed
// row by row and injected at the level with as many nodes as it has rows.
// Every level runs on the GPU; commit_device (merkle.cpp), the prover's path,
// is not involved.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <functional>

#include "host.hpp"
#include "host_slice.hpp"
#include "prove_internal.hpp"

namespace lsp {

std::vector<HeightClass> height_classes(const size_t* widths, const size_t* heights, size_t nmats) {
    LSP_REQUIRE(widths && heights && nmats >= 1, LSP_E_ARG, "a batch needs at least one matrix");
    std::vector<size_t> order(nmats);
    for (size_t k = 0; k < nmats; ++k) {
        LSP_REQUIRE(widths[k] >= 1 && widths[k] <= ((size_t)1 << 20), LSP_E_ARG, "matrix width outside [1, 2^20]");
        LSP_REQUIRE(heights[k] <= ((size_t)1 << 40), LSP_E_SIZE, "matrix height beyond 2^40");
        log2_exact(heights[k]);
        // (at most 2^60 here) so that no byte count below overflows
        LSP_REQUIRE(heights[k] * widths[k] <= ((size_t)1 << 48), LSP_E_SIZE, "matrix beyond 2^48 elements");
        order[k] = k;
    }
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return heights[a] > heights[b]; });
    std::vector<HeightClass> cls;
    for (size_t k : order) {
        if (cls.empty() || cls.back().height != heights[k]) cls.push_back({heights[k], {}});
        LSP_REQUIRE(cls.back().idx.size() < 8, LSP_E_ARG, "more than 8 matrices of one height");
        cls.back().idx.push_back(k);
    }
    return cls;
}

}  // namespace lsp

lsp_tree::~lsp_tree() {
    if (ctx->device != LSP_HOST_ONLY) (void)hipSetDevice(ctx->device);
    for (auto* d : mats) (void)hipFree(d);
    (void)hipFree(layers);
}

namespace lsp {

static Fr* dev_alloc_fr(size_t n, const char* what) {
    Fr* d = nullptr;
    if (hipMalloc(&d, n * sizeof(Fr)) != hipSuccess) {
        (void)hipGetLastError();
        throw LspError(LSP_E_OOM, std::string("hipMalloc of ") + what + " failed");
    }
    return d;
}

std::unique_ptr<lsp_tree> new_tree(lsp_ctx* ctx, size_t leaves, size_t nmats, const size_t* heights,
                                   const size_t* widths, const lsp_fr* const* src, int mem) {
    auto t = std::make_unique<lsp_tree>(ctx, leaves);
    t->widths.assign(widths, widths + nmats);
    t->heights.assign(heights, heights + nmats);
    for (size_t k = 0; k < nmats; ++k) {
        const size_t n = heights[k] * widths[k];
        t->mats.push_back(dev_alloc_fr(n, "a tree's matrix"));
        if (src)
            LSP_HIP(hipMemcpyAsync(t->mats[k], src[k], n * sizeof(Fr),
                                   mem == LSP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                   ctx->stream));
    }
    t->layers = dev_alloc_fr(TreeLayout{leaves}.size(), "a tree's layers");
    return t;
}

// The host slice of a mixed tree (host_slice.hpp), only where LSP_HOST_SLICE
// forces one: no proof commits through here, and the caller of the C API may be
// using the host.  The host's subtree -- the last leaves >> log_frac leaves, with
// its share of every class at least 2^log_frac rows high -- ends in its single
// root, in the layer of 2^log_frac nodes; the GPU's levels run on prefixes down
// to that layer, take the host's layers in behind them, and go on whole.
static HostSlice mixed_slice(size_t leaves) {
    HostSliceIn in;
    const char* e = std::getenv("LSP_HOST_SLICE");
    in.forced = e ? (int)std::strtol(e, nullptr, 10) : 0;
    if (in.forced <= 0 || in.forced >= 40) return {};
    in.leaves = leaves;
    in.join = (size_t)1 << in.forced;
    return plan_host_slice(in);
}

namespace {
struct MixedSlice {
    HostSlice hs;
    size_t S = 0;                  // the slice's leaves
    Fr* buf = nullptr;             // pinned: the subtree's layers (TreeLayout{S}), then the rows
    std::vector<const Fr*> rows;   // per matrix, the caller's index: its rows in the slice (host), or none
};
}  // namespace

// the slice's rows of every class into pinned memory, on the side stream
static MixedSlice mixed_slice_download(lsp_ctx* ctx, const std::vector<HeightClass>& cls, const Fr* const* mats,
                                       const size_t* widths, HostSlice hs) {
    MixedSlice s;
    s.hs = hs;
    s.S = hs.slice(cls[0].height);
    size_t elems = 0, nmats = 0;
    for (const HeightClass& c : cls)
        for (size_t k : c.idx) {
            elems += hs.slice(c.height) * widths[k];
            nmats = std::max(nmats, k + 1);
        }
    s.rows.assign(nmats, nullptr);
    s.buf = (Fr*)ctx->hbuf("merkle_mixed_slice", (TreeLayout{s.S}.size() + elems) * sizeof(Fr));
    hipStream_t sd = slice_stream_begin(ctx);
    Fr* dst = s.buf + TreeLayout{s.S}.size();
    for (const HeightClass& c : cls) {
        const size_t n = hs.slice(c.height);  // (0: the class enters above the slice's root)
        for (size_t k : c.idx) {
            if (!n) continue;
            LSP_HIP(hipMemcpyAsync(dst, mats[k] + (c.height - n) * widths[k], n * widths[k] * sizeof(Fr),
                                   hipMemcpyDeviceToHost, sd));
            s.rows[k] = dst;
            dst += n * widths[k];
        }
    }
    slice_stream_end(ctx);
    return s;
}

// the slice's subtree on the host pool, level by level with every class
// injected where the GPU injects it; its layers then go into the suffix of
// each device layer, on the context's stream
static void mixed_slice_hash(lsp_ctx* ctx, const std::vector<HeightClass>& cls, const size_t* widths,
                             const MixedSlice& s, Fr* layers) {
    LSP_HIP(hipEventSynchronize(ctx->ev_slice));
    HostPool& pool = ctx->host_pool();
    const TreeLayout lay{cls[0].height}, sl{s.S};
    auto chunks = [&](size_t n, const std::function<void(size_t, size_t)>& f) {
        pool.parallel_for((n + 63) / 64, [&](size_t b) { f(64 * b, std::min(n, 64 * b + 64)); });
    };
    auto class_digests = [&](const HeightClass& c, Fr* out, size_t n) {
        const Fr* rows[8];
        size_t w[8];
        for (size_t j = 0; j < c.idx.size(); ++j) {
            rows[j] = s.rows[c.idx[j]];
            w[j] = widths[c.idx[j]];
        }
        chunks(n, [&](size_t i0, size_t i1) { host_hash_rows(ctx->p2, rows, w, c.idx.size(), out, i0, i1); });
    };
    class_digests(cls[0], s.buf, s.S);
    std::vector<Fr> inj;
    size_t next = 1;
    for (uint32_t j = 1; j <= sl.levels(); ++j) {
        const Fr* in = s.buf + sl.offset(j - 1);
        Fr* out = s.buf + sl.offset(j);
        const size_t nout = sl.len(j);
        chunks(nout, [&](size_t i0, size_t i1) { ctx->p2.compress_range(in, out, i0, i1); });
        if (next < cls.size() && cls[next].height == lay.len(j)) {
            inj.resize(nout);
            class_digests(cls[next++], inj.data(), nout);
            chunks(nout, [&](size_t i0, size_t i1) {
                for (size_t i = i0; i < i1; ++i) out[i] = ctx->p2.compress(out[i], inj[i]);
            });
        }
    }
    for (uint32_t j = 0; j <= sl.levels(); ++j)
        LSP_HIP(hipMemcpyAsync(layers + lay.offset(j) + s.hs.prefix(lay.len(j)), s.buf + sl.offset(j),
                               sl.len(j) * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
}

Fr commit_mixed_device(lsp_ctx* ctx, const std::vector<HeightClass>& cls, const Fr* const* mats, const size_t* widths,
                       Fr* layers) {
    hipStream_t st = ctx->stream;
    const TreeLayout lay{cls[0].height};
    const HostSlice hs = mixed_slice(lay.leaves);
    MixedSlice sl;
    if (hs) sl = mixed_slice_download(ctx, cls, mats, widths, hs);
    // every class's row digests, into the layer they enter: the leaves for the
    // tallest class, for the others the layer the injecting level then
    // overwrites in place.  The levels' dependent chain holds no sponge.
    for (const HeightClass& c : cls) {
        MatList m{};
        m.n = (uint32_t)c.idx.size();
        for (uint32_t j = 0; j < m.n; ++j) {
            m.ptr[j] = mats[c.idx[j]];
            m.width[j] = (uint32_t)widths[c.idx[j]];
        }
        LSP_HIP(launch_hash_rows(m, hs.prefix(c.height), layers + lay.offset_of_len(c.height), ctx->rc29_dev,
                                 ctx->p2.L, st));
    }
    size_t off = 0, len = lay.leaves, next = 1;
    if (hs) {
        // the GPU's prefix of every level down to the layer of the slice's root
        while (hs.slice(len / 2) >= 1) {
            const size_t nout = len / 2;
            Fr* dst = layers + off + len;
            if (next < cls.size() && cls[next].height == nout) {
                LSP_HIP(launch_merkle_inject(layers + off, dst, dst, hs.prefix(nout), ctx->rc29_dev, ctx->p2.L, st));
                ++next;
            } else
                LSP_HIP(launch_merkle_level(layers + off, dst, hs.prefix(nout), ctx->rc29_dev, ctx->p2.L, st));
            off += len;
            len = nout;
        }
        mixed_slice_hash(ctx, cls, widths, sl, layers);
    }
    while (len > 1) {
        if (next == cls.size()) {  // no class left: the plain tree, its one-workgroup top included
            LSP_HIP(launch_merkle_tree(layers + off, len, ctx->rc29_dev, ctx->p2.L, st));
            break;
        }
        const size_t nout = len / 2;
        Fr* dst = layers + off + len;
        if (cls[next].height == nout) {
            LSP_HIP(launch_merkle_inject(layers + off, dst, dst, nout, ctx->rc29_dev, ctx->p2.L, st));
            ++next;
        } else
            LSP_HIP(launch_merkle_level(layers + off, dst, nout, ctx->rc29_dev, ctx->p2.L, st));
        off += len;
        len = nout;
    }
    return d2h_fr(ctx, layers + lay.root());
}

bool verify_mixed_host(const lsp_ctx* ctx, const Fr& root, const std::vector<HeightClass>& cls, const size_t* widths,
                       size_t nmats, size_t index, const lsp_fr* rows, const lsp_fr* path) {
    std::vector<size_t> at(nmats + 1, 0);  // matrix k's row starts at rows[at[k]] (the caller's order)
    for (size_t k = 0; k < nmats; ++k) at[k + 1] = at[k] + widths[k];
    auto class_hash = [&](const HeightClass& c) {
        std::vector<Fr> v;
        for (size_t k : c.idx)
            for (size_t e = at[k]; e < at[k + 1]; ++e) v.push_back(to_fr(rows[e]));
        return ctx->p2.hash(v.data(), v.size());
    };
    const TreeLayout lay{cls[0].height};
    size_t next = 1;
    const Fr got = merkle_path_root(
        ctx->p2, class_hash(cls[0]), index, lay.levels(), [&](uint32_t l) { return to_fr(path[l]); },
        [&](uint32_t level, const Fr& cur) {
            if (next == cls.size() || cls[next].height != lay.len(level)) return cur;
            return ctx->p2.compress(cur, class_hash(cls[next++]));
        });
    return fr_eq(got, root);
}

}  // namespace lsp
