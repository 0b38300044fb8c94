// Host helpers: field constants, AIR descriptor parsing and symbolic degrees,
// device buffer pool, twiddle cache.
#include "host.hpp"

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdlib>
#include <cstring>

#if defined(__linux__)
#include <sched.h>
#endif

#include "comm.hpp"  // ~lsp_ctx deletes its communicator

namespace lsp {

Fr host_generator() { return fr_from_u64(22); }

Fr host_inv_cached(const Fr& a) {
    static std::mutex mu;
    static std::map<std::array<uint32_t, 8>, Fr> cache;
    std::array<uint32_t, 8> k;
    for (int i = 0; i < 8; ++i) k[i] = a.v[i];
    {
        std::lock_guard<std::mutex> g(mu);
        auto it = cache.find(k);
        if (it != cache.end()) return it->second;
    }
    const Fr r = fr_inv(a);
    std::lock_guard<std::mutex> g(mu);
    if (cache.size() > 4096) cache.clear();
    cache[k] = r;
    return r;
}

Fr host_two_adic_generator(uint32_t bits) {
    // ROOT_2_47 = 22^((r-1) >> 47); (r-1) >> 47 as 32-bit words
    static Fr root47 = [] {
        // r - 1 = 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000000
        uint32_t e[8] = {0x00000000u, 0x0a118000u, 0xd0000001u, 0x59aa76feu,
                         0x5c37b001u, 0x60b44d1eu, 0x9a2ca556u, 0x12ab655eu};
        // shift right by 47 bits: one word (32) + 15 bits
        uint32_t s[8] = {0};
        for (int i = 0; i < 7; ++i) s[i] = e[i + 1];
        uint32_t t[8] = {0};
        for (int i = 0; i < 8; ++i) t[i] = (s[i] >> 15) | (i + 1 < 8 ? (s[i + 1] << 17) : 0u);
        Fr g = fr_from_u64(22), r = fr_one();
        bool started = false;
        for (int w = 7; w >= 0; --w)
            for (int k = 31; k >= 0; --k) {
                if (started) r = fr_sqr(r);
                if ((t[w] >> k) & 1u) {
                    r = started ? fr_mul(r, g) : g;
                    started = true;
                }
            }
        return r;
    }();
    if (bits > 47) throw LspError(LSP_E_SIZE, "two-adicity of Fr is 47");
    Fr r = root47;
    for (uint32_t k = bits; k < 47; ++k) r = fr_sqr(r);
    return r;
}

uint64_t host_bitrev(uint64_t x, uint32_t bits) {
    uint64_t r = 0;
    for (uint32_t i = 0; i < bits; ++i) {
        r = (r << 1) | (x & 1);
        x >>= 1;
    }
    return r;
}

uint32_t log2_exact(size_t n) {
    uint32_t b = 0;
    while (((size_t)1 << b) < n) ++b;
    if (n == 0 || ((size_t)1 << b) != n) throw LspError(LSP_E_SIZE, "height must be a power of two");
    return b;
}

HostPool::HostPool(unsigned workers) {
    for (unsigned i = 0; i < workers; ++i) th_.emplace_back([this] { loop(); });
}

HostPool::~HostPool() {
    {
        std::lock_guard<std::mutex> lk(m_);
        stop_.store(true);
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
}

static inline void cpu_relax() {
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
}

void HostPool::loop() {
    uint64_t seen = 0;
    for (;;) {
        // spin for a new generation, then sleep
        const auto t0 = std::chrono::steady_clock::now();
        const int64_t until = std::max<int64_t>(
            std::chrono::duration_cast<std::chrono::nanoseconds>((t0 + std::chrono::microseconds(kSpinUs)).time_since_epoch())
                .count(),
            spin_until_ns_.load(std::memory_order_relaxed));
        for (unsigned it = 0; gen_.load() == seen && !stop_.load(); ++it) {
            cpu_relax();
            if ((it & 255) == 255 &&
                std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
                        .count() > until) {
                std::unique_lock<std::mutex> lk(m_);
                sleepers_.fetch_add(1);  // seq_cst: pairs with parallel_for's gen_ / sleepers_ order
                cv_.wait(lk, [&] { return stop_.load() || gen_.load() != seen; });
                sleepers_.fetch_sub(1);
                break;
            }
        }
        if (stop_.load()) return;
        seen = gen_.load();
        const auto* job = job_;
        const size_t n = n_;
        for (size_t i; (i = next_.fetch_add(1)) < n;) (*job)(i);
        busy_.fetch_sub(1);
    }
}

void HostPool::wake(unsigned spin_us) {
    if (th_.empty()) return;
    if (spin_us)
        spin_until_ns_.store(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                 (std::chrono::steady_clock::now() + std::chrono::microseconds(spin_us)).time_since_epoch())
                                 .count(),
                             std::memory_order_relaxed);
    while (busy_.load() != 0) cpu_relax();
    job_ = nullptr;
    n_ = 0;
    next_.store(0);
    busy_.store((unsigned)th_.size());
    gen_.fetch_add(1);
    if (sleepers_.load() != 0) {
        std::lock_guard<std::mutex> lk(m_);
        cv_.notify_all();
    }
}

void HostPool::parallel_for(size_t n, const std::function<void(size_t)>& f) {
    if (th_.empty() || n < 2) {
        for (size_t i = 0; i < n; ++i) f(i);
        return;
    }
    while (busy_.load() != 0) cpu_relax();  // a wake() may still be draining
    // the previous job has fully drained (busy_ == 0), so no worker reads these
    job_ = &f;
    n_ = n;
    next_.store(0);
    busy_.store((unsigned)th_.size());
    gen_.fetch_add(1);
    if (sleepers_.load() != 0) {
        std::lock_guard<std::mutex> lk(m_);
        cv_.notify_all();
    }
    for (size_t i; (i = next_.fetch_add(1)) < n;) f(i);
    for (unsigned it = 0; busy_.load() != 0; ++it) {
        cpu_relax();
        if ((it & 4095) == 4095) std::this_thread::yield();
    }
}

Fr P2Host::hash(const Fr* in, size_t n) const {
    Fr s0 = fr_zero(), s1 = fr_zero(), s2 = fr_zero();
    size_t k = 0;
    while (k + 2 <= n) {
        s0 = in[k];
        s1 = in[k + 1];
        permute(s0, s1, s2);
        k += 2;
    }
    if (k < n) {
        s0 = in[k];
        permute(s0, s1, s2);
    }
    return s0;
}

// ------------------------------------------------------------------- AIR
// An LSP_AIR_PROGRAM config (include/lsp.h) after its type word.  Everything a
// kernel later indexes with -- slots, constants, columns, public values -- is
// checked here or in require_fits, and a slot is read only after an earlier op
// wrote it, so no evaluator ever sees an undefined register.
// prep: an LSP_AIR_PROGRAM_PREP config -- prep_width follows width, and the
// operand kinds PREP_LOCAL / PREP_NEXT exist.  Its device form is a plain
// program's (type word 3, no prep_width: the kernels take the matrix's width
// from the launch), so both types share the interpreter.
template <class Next>
static void parse_program(Air& air, AirCfg& g, Next&& next, size_t cfg, bool prep) {
    const int32_t width = next(), prep_width = prep ? next() : 0;
    const int32_t nslots = next(), nconst = next(), nops = next(), nassert = next();
    const std::string where = "AIR program (config " + std::to_string(cfg) + ")";
    LSP_REQUIRE(width >= 1 && width <= (1 << 20), LSP_E_ARG, where + ": bad width");
    LSP_REQUIRE(!prep || (prep_width >= 1 && prep_width <= (1 << 20)), LSP_E_ARG,
                where + ": preprocessed width outside [1, 2^20]");
    air.prep_width = std::max(air.prep_width, (uint32_t)prep_width);
    LSP_REQUIRE(nslots >= 0 && nslots <= (int32_t)AIR_PROG_MAX_SLOTS, LSP_E_ARG, where + ": more than 16 slots");
    LSP_REQUIRE(nconst >= 0 && nconst <= (1 << 16), LSP_E_ARG, where + ": more than 2^16 constants");
    LSP_REQUIRE(nops >= 1 && nops <= (1 << 20), LSP_E_ARG, where + ": op count outside [1, 2^20]");
    LSP_REQUIRE(nassert >= 1 && nassert <= nops, LSP_E_ARG, where + ": bad assert count");
    air.has_prog = true;
    air.prog_slots = std::max(air.prog_slots, (uint32_t)nslots);
    air.dev.insert(air.dev.end(), {LSP_AIR_PROGRAM, width, nslots, nconst, nops, nassert});
    for (int32_t i = 0; i < nconst; ++i) {
        Fr c;
        for (int k = 0; k < 8; ++k) c.v[k] = (uint32_t)next();
        LSP_REQUIRE(fr_words_lt_mod(c), LSP_E_ARG, where + ": constant " + std::to_string(i) + " is not below r");
        const Fr m = fr_from_canonical(c);
        g.pconst.push_back(m);
        // the device's form: the nine 29-bit limbs of c 2^261 mod r (fr29.hpp), canonical
        const Fr x = fr_mul(m, fr_from_u64(32));
        for (int l = 0; l < 9; ++l) {
            const int bit = 29 * l, wd = bit >> 5, sh = bit & 31;
            uint64_t v = x.v[wd];
            if (wd + 1 < 8) v |= (uint64_t)x.v[wd + 1] << 32;
            air.dev.push_back((int32_t)((uint32_t)(v >> sh) & (l < 8 ? 0x1fffffffu : 0xffffffffu)));
        }
    }
    uint32_t written = 0, asserts = 0;  // slots written so far, a bit each
    for (int32_t i = 0; i < nops; ++i) {
        const std::string op = where + " op " + std::to_string(i);
        const int32_t code = next(), dst = next(), a = next(), b = next();
        auto operand = [&](int32_t x) {
            const uint32_t kind = (uint32_t)x >> 24, v = (uint32_t)x & 0xffffffu;
            switch (kind) {
                case AIR_OPND_SLOT:
                    LSP_REQUIRE(v < (uint32_t)nslots, LSP_E_ARG, op + ": slot past nslots");
                    LSP_REQUIRE(written >> v & 1, LSP_E_ARG, op + ": slot read before it is written");
                    break;
                case AIR_OPND_LOCAL:
                case AIR_OPND_NEXT:
                    LSP_REQUIRE(v < (uint32_t)width, LSP_E_ARG, op + ": column outside the program's width");
                    air.max_col = std::max(air.max_col, v);
                    break;
                case AIR_OPND_PUBLIC:
                    LSP_REQUIRE(v < (1u << 16), LSP_E_ARG, op + ": public index 2^16 or more");
                    air.max_pub = std::max<int64_t>(air.max_pub, v);
                    break;
                case AIR_OPND_CONST:
                    LSP_REQUIRE(v < (uint32_t)nconst, LSP_E_ARG, op + ": constant past nconst");
                    break;
                case AIR_OPND_FIRST:
                case AIR_OPND_LAST:
                case AIR_OPND_TRANS:
                    LSP_REQUIRE(v == 0, LSP_E_ARG, op + ": selector operand with a payload");
                    break;
                case AIR_OPND_PREP_LOCAL:
                case AIR_OPND_PREP_NEXT:
                    LSP_REQUIRE(prep, LSP_E_ARG, op + ": unknown operand kind (preprocessed cells need config type 4)");
                    LSP_REQUIRE(v < (uint32_t)prep_width, LSP_E_ARG,
                                op + ": column outside the program's preprocessed width");
                    break;
                default: throw LspError(LSP_E_ARG, op + ": unknown operand kind");
            }
        };
        if (code == AIR_OP_ASSERT_ZERO) {
            LSP_REQUIRE(dst == 0 && b == 0, LSP_E_ARG, op + ": nonzero unused field");
            operand(a);
            ++asserts;
        } else {
            LSP_REQUIRE(code == AIR_OP_ADD || code == AIR_OP_SUB || code == AIR_OP_MUL, LSP_E_ARG,
                        op + ": unknown opcode");
            LSP_REQUIRE(dst >= 0 && dst < nslots, LSP_E_ARG, op + ": destination past nslots");
            operand(a);
            operand(b);
            written |= 1u << dst;
        }
        g.pops.insert(g.pops.end(), {code, dst, a, b});
    }
    LSP_REQUIRE(asserts == (uint32_t)nassert, LSP_E_ARG, where + ": nassert is not the number of ASSERT_ZERO ops");
    air.dev.insert(air.dev.end(), g.pops.begin(), g.pops.end());
}

Air Air::parse(const int32_t* d, size_t n) {
    Air air;
    LSP_REQUIRE(d && n >= 1, LSP_E_ARG, "empty AIR descriptor");
    LSP_REQUIRE(n <= (size_t)INT32_MAX, LSP_E_ARG, "AIR descriptor of 2^31 words or more");
    air.raw.assign(d, d + n);
    // air_decode's reader over words nobody has checked yet
    struct {
        const int32_t* d;
        size_t n, p;
        int32_t word() {
            LSP_REQUIRE(p < n, LSP_E_ARG, "truncated AIR descriptor");
            return d[p++];
        }
        const int32_t* words(int64_t k) {
            LSP_REQUIRE(k >= 0 && (uint64_t)k <= n - p, LSP_E_ARG, "truncated AIR descriptor");
            p += (size_t)k;
            return d + p - k;
        }
    } r{d, n, 0};
    auto cols = [&](const int32_t* ids, int64_t k) {
        for (int64_t i = 0; i < k; ++i) {
            LSP_REQUIRE(ids[i] >= 0 && ids[i] < (1 << 20), LSP_E_ARG, "bad column id in AIR descriptor");
            air.max_col = std::max(air.max_col, (uint32_t)ids[i]);
        }
    };
    auto count = [](int32_t k) { return k >= 1 && k <= 4096; };
    const int32_t nc = r.word();
    LSP_REQUIRE(nc >= 1 && nc <= 4096, LSP_E_ARG, "bad config count in AIR descriptor");
    air.dev.push_back(nc);
    for (int32_t c = 0; c < nc; ++c) {
        AirCfg g;
        const size_t p0 = r.p;
        g.type = r.word();
        g.off = (int32_t)r.p;
        if (g.type == LSP_AIR_PERMUTATION || g.type == LSP_AIR_LOOKUP) {
            const AirView v = air_decode(g.type, r);
            if (g.type == LSP_AIR_PERMUTATION) {
                LSP_REQUIRE(count(v.na) && count(v.nbc), LSP_E_ARG, "bad permutation widths");
            } else {
                LSP_REQUIRE(count(v.na), LSP_E_ARG, "bad lookup A width");
                LSP_REQUIRE(count(v.ntab) && count(v.nbc), LSP_E_ARG, "bad lookup B tables");
                cols(&v.a_filter, 1);
                cols(v.b_filter, v.ntab);
                cols(&v.a_inv, 1);
                cols(v.occ, v.ntab);
            }
            cols(v.a, v.na);
            cols(v.b, (int64_t)v.ntab * v.nbc);
            cols(v.b_inv, v.ntab);
            cols(&v.check, 1);
            air.dev.insert(air.dev.end(), d + p0, d + r.p);
        } else if (g.is_prog()) {
            // (appends its device form to air.dev)
            parse_program(air, g, [&] { return r.word(); }, (size_t)c, g.type == LSP_AIR_PROGRAM_PREP);
        } else {
            throw LspError(LSP_E_ARG, "unknown AIR config type");
        }
        air.cfgs.push_back(std::move(g));
    }
    LSP_REQUIRE(r.p == n, LSP_E_ARG, "trailing data in AIR descriptor");
    return air;
}

void Air::require_fits(size_t w, size_t npub, size_t wp) const {
    LSP_REQUIRE(npub >= 2, LSP_E_ARG, "public values must hold [alpha, delta]");
    LSP_REQUIRE(prep_width == 0 || wp != 0, LSP_E_ARG,
                "the AIR reads preprocessed columns: this call has no preprocessed matrix");
    LSP_REQUIRE(prep_width <= wp, LSP_E_ARG,
                "the AIR reads " + std::to_string(prep_width) + " preprocessed columns of " + std::to_string(wp));
    LSP_REQUIRE(max_col < w, LSP_E_ARG, "AIR column id outside the trace width");
    LSP_REQUIRE(max_pub < (int64_t)npub, LSP_E_ARG,
                "AIR program reads public value " + std::to_string(max_pub) + " of " + std::to_string(npub));
}

// Symbolic degree_multiple rules of p3-uni-stark as an algebra: main and
// preprocessed variables 1, constants 0, public values `pd` (U6), IsFirstRow /
// IsLastRow 1, IsTransition 0; Add / Sub max, Mul sum (saturating: 2^20
// squarings would overflow, and any such degree is far past every blowup).
namespace {
struct DegAlgebra {
    using V = int;
    int zero() const { return 0; }
    int one() const { return 0; }
    int add(int a, int b) const { return std::max(a, b); }
    int sub(int a, int b) const { return std::max(a, b); }
    int mul(int a, int b) const { return (int)std::min<int64_t>((int64_t)a + b, 1 << 30); }
    int load(const void*, int32_t) const { return 1; }
};
template <Sel S>
constexpr int sel_degree(SelTag<S>) {
    return S == Sel::First || S == Sel::Last ? 1 : 0;
}
}  // namespace

// walk(cfg index, degree of the constraint with its selector, what it is) over the whole AIR
template <class F>
static void walk_degrees(const Air& air, int pd, F&& f) {
    const DegAlgebra D;
    auto leaf = [&](const AirCfg&, uint32_t k, uint32_t) {
        return k == AIR_OPND_PUBLIC ? pd : k == AIR_OPND_CONST || k == AIR_OPND_TRANS ? 0 : 1;
    };
    for (size_t c = 0; c < air.cfgs.size(); ++c)
        air.walk(D, air.cfgs[c], nullptr, nullptr, pd, pd, leaf,
                 [&](int v, auto sel, AirCons what) { f(c, D.mul(sel_degree(sel), v), what); });
}

std::vector<int> Air::degrees(int pd) const {
    std::vector<int> out;
    walk_degrees(*this, pd, [&](size_t, int deg, AirCons) { out.push_back(deg); });
    return out;
}

std::pair<int, int> Air::stats(int pd) const {
    const std::vector<int> d = degrees(pd);
    return {d.empty() ? 0 : *std::max_element(d.begin(), d.end()), (int)d.size()};
}

uint32_t Air::log_quotient_degree(int pd) const {
    int d = std::max(stats(pd).first, 2);
    uint32_t lg = 0;
    while ((1 << lg) < d - 1) ++lg;
    return lg;
}

void Air::eval_fold(const Fr* loc, const Fr* nxt, const Fr* pub, const Fr& first, const Fr& last, const Fr& trans,
                    const Fr& al, Fr& acc, const Fr* ploc, const Fr* pnxt) const {
    eval(loc, nxt, pub, first, last, trans, [&](const Fr& x) { acc = fr_add(fr_mul(acc, al), x); }, ploc, pnxt);
}

Air::ConsInfo Air::constraint_info(uint32_t j) const {
    ConsInfo o{};
    uint32_t k = 0;
    walk_degrees(*this, 0, [&](size_t c, int, AirCons what) {
        if (k++ == j) o = ConsInfo{(uint32_t)c, cfgs[c].type, what.kind, what.table};
    });
    LSP_REQUIRE(j < k, LSP_E_ARG, "constraint index past the AIR's last constraint");
    return o;
}

}  // namespace lsp

// ------------------------------------------------------------------ context
// Also a half-built context's (lsp_ctx_create): the stream is the first thing
// made on the device, so without one there is nothing else to release.
lsp_ctx::~lsp_ctx() {
    delete comm;
    if (device == LSP_HOST_ONLY || !stream) return;
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);
    if (side_stream) (void)hipStreamSynchronize(side_stream);
    for (auto& kv : pool)
        if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto& kv : hpool)
        if (kv.second.p) (void)hipHostFree(kv.second.p);
    for (auto& kv : stage_ev) (void)hipEventDestroy(kv.second);
    for (hipEvent_t e : event_pool) (void)hipEventDestroy(e);
    for (auto& t : pending_timings) {
        (void)hipEventDestroy(std::get<1>(t));
        (void)hipEventDestroy(std::get<2>(t));
    }
    if (ev_near) (void)hipEventDestroy(ev_near);
    if (ev_top) (void)hipEventDestroy(ev_top);
    if (ev_warm) (void)hipEventDestroy(ev_warm);
    if (ev_slice_in) (void)hipEventDestroy(ev_slice_in);
    if (ev_slice) (void)hipEventDestroy(ev_slice);
    if (ev_slice_up) (void)hipEventDestroy(ev_slice_up);
    if (side_stream) {
        (void)hipStreamSynchronize(side_stream);
        (void)hipEventDestroy(ev_wide);
        (void)hipEventDestroy(ev_side);
        (void)hipStreamDestroy(side_stream);
    }
    if (rc_dev) (void)hipFree(rc_dev);
    if (rc29_dev) (void)hipFree(rc29_dev);
    (void)hipStreamDestroy(stream);
}

void* lsp_ctx::buf(const std::string& name, size_t bytes) {
    Buf& b = pool[name];
    if (b.cap < bytes) {
        if (b.p) {
            LSP_HIP(hipStreamSynchronize(stream));
            LSP_HIP(hipFree(b.p));
            b.p = nullptr;
            b.cap = 0;
        }
        if (bytes) {
            hipError_t e = hipMalloc(&b.p, bytes);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                throw lsp::LspError(LSP_E_OOM, "hipMalloc(" + std::to_string(bytes) + ") for " + name + " failed");
            }
            b.cap = bytes;
        }
    }
    return b.p;
}

void lsp_ctx::release(const std::string& prefix) {
    LSP_HIP(hipStreamSynchronize(stream));
    for (auto it = pool.begin(); it != pool.end();) {
        if (it->first.compare(0, prefix.size(), prefix) == 0) {
            if (it->second.p) LSP_HIP(hipFree(it->second.p));
            it = pool.erase(it);
        } else {
            ++it;
        }
    }
}

void* lsp_ctx::hbuf(const std::string& name, size_t bytes, unsigned flags) {
    Buf& b = hpool[name];
    if (b.cap < bytes) {
        if (b.p) {
            LSP_HIP(hipStreamSynchronize(stream));
            LSP_HIP(hipHostFree(b.p));
            b.p = nullptr;
            b.cap = 0;
        }
        if (bytes) {
            if (hipHostMalloc(&b.p, bytes, flags ? flags : hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                throw lsp::LspError(LSP_E_OOM, "hipHostMalloc(" + std::to_string(bytes) + ") for " + name + " failed");
            }
            b.cap = bytes;
        }
    }
    return b.p;
}

void lsp_ctx::h2d_async(const std::string& name, void* dst, const void* src, size_t bytes) {
    if (!bytes) return;
    auto it = stage_ev.find(name);
    if (it == stage_ev.end()) {
        hipEvent_t ev;
        LSP_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        it = stage_ev.emplace(name, ev).first;
    } else {
        LSP_HIP(hipEventSynchronize(it->second));
    }
    void* h = hbuf(name, bytes);
    std::memcpy(h, src, bytes);
    LSP_HIP(hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, stream));
    LSP_HIP(hipEventRecord(it->second, stream));
}

hipStream_t lsp_ctx::side() {
    if (!side_stream) {
        int least = 0, greatest = 0;
        LSP_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        LSP_HIP(hipStreamCreateWithPriority(&side_stream, hipStreamNonBlocking, least));
        LSP_HIP(hipEventCreateWithFlags(&ev_wide, hipEventDisableTiming));
        LSP_HIP(hipEventCreateWithFlags(&ev_side, hipEventDisableTiming));
    }
    return side_stream;
}

lsp::HostPool& lsp_ctx::host_pool() {
    if (!pool_) {
        pool_.reset(new lsp::HostPool(lsp::default_host_threads() - 1));
    }
    return *pool_;
}

// The host pool's size: up to 16 threads (a 1-GPU box's CPU share).  The CPUs
// counted are this process's affinity set (hardware_concurrency() counts the
// whole machine: 256 on a box whose GPU share is 16).  When the launcher says
// several ranks share this host (torchrun's LOCAL_WORLD_SIZE), the set is
// divided among them: the library cannot tell a set the ranks share from a
// slice a launcher pinned for this rank alone, and of the two mistakes
// dividing a private slice only makes the pool smaller, while not dividing a
// shared one puts ranks x 16 spinning threads on it.  The Python
// launch path (replicas.init_from_env) compares the ranks' sets and exports
// the exact size as LSP_HOST_THREADS, which overrides this; other launchers
// that pin each rank to its own CPUs set LSP_HOST_THREADS themselves (lsp.h).
unsigned lsp::default_host_threads() {
    unsigned ranks = 1;
    if (const char* e = std::getenv("LOCAL_WORLD_SIZE")) ranks = (unsigned)std::max(1L, std::strtol(e, nullptr, 10));
    unsigned cpus = std::max(1u, std::thread::hardware_concurrency());
#if defined(__linux__)
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) > 0) cpus = (unsigned)CPU_COUNT(&set);
#endif
    unsigned n = std::min(16u, std::max(1u, cpus / ranks));
    if (const char* e = std::getenv("LSP_HOST_THREADS")) n = (unsigned)std::max(1L, std::strtol(e, nullptr, 10));
    return n;
}

const lsp::Fr* lsp_ctx::table(const std::string& key, size_t n, const std::function<void(lsp::Fr*)>& fill,
                              const char* scratch) {
    const auto it = key.empty() ? tables.end() : tables.find(key);
    if (it != tables.end()) return it->second;
    const bool keep = !key.empty() && (!scratch || tables.size() < 256);
    lsp::Fr* tab = fbuf(keep ? key : std::string(scratch), n);
    fill(tab);
    LSP_HIP(hipStreamSynchronize(stream));  // the fill's host temporaries may die now
    if (keep) tables[key] = tab;
    return tab;
}

void lsp_ctx::sync() { LSP_HIP(hipStreamSynchronize(stream)); }
