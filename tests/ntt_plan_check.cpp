// The invariants of the coset LDE's pass plan (csrc/ntt_plan.hpp), checked on
// the host alone: built and run by tests/test_ntt_plan.py.  Prints one line per
// broken invariant and exits nonzero if there is any.
#include <cstdio>
#include <vector>

#include "ntt_plan.hpp"

using namespace lsp;

static int failures = 0;
static const char* ctx_what;
static uint32_t ctx_logh, ctx_w, ctx_nc;
static int ctx_knobs, ctx_rf;

#define CHECK(cond)                                                                                              \
    do {                                                                                                         \
        if (!(cond) && ++failures <= 40)                                                                         \
            std::printf("FAIL %s logh=%u w=%u cosets=%u knobs=%d row_factors=%d: %s\n", ctx_what, ctx_logh, ctx_w, \
                        ctx_nc, ctx_knobs, ctx_rf, #cond);                                                       \
    } while (0)

// the LDS bytes k_ntt_rm carves out: the tile, the fused pass's row factors and
// (16-byte aligned) twiddle cache, the plain passes' reduction table
static size_t lds_parts(const PlannedPass& p, bool row_factors) {
    const bool fused = p.mode == PASS_INV_FWD;
    const size_t rows = (size_t)1 << (p.k + p.logG), n_el = rows << p.logCW;
    size_t b = n_el * 36;
    if (fused && row_factors) b += rows * 36;
    if (p.twl_n) b = ((b + 15) / 16) * 16 + (size_t)p.twl_n * 48;
    if (!fused) b += 64 * 48;
    return b;
}

static void check_pass(const PlannedPass& p, uint32_t logh, uint32_t w, uint32_t nc, bool rf, const NttKnobs& kn) {
    const bool fused = p.mode == PASS_INV_FWD;
    CHECK(p.k >= 1 && p.k <= 10);
    CHECK(p.k + p.logG + p.logCW <= 10);  // at most 1024 elements
    CHECK(((size_t)1 << (p.k + p.logG + p.logCW)) <= NTT_MAX_EL);
    CHECK(p.logG <= logh - p.k);
    CHECK(p.logCW <= 3);
    CHECK(p.twl_n <= 512);
    CHECK(fused || p.twl_n == 0);
    const size_t twl_all = ((size_t)1 << p.logG) * (((size_t)1 << p.k) - 1);
    CHECK(p.twl_n == (fused && kn.twl && twl_all <= 512 ? twl_all : 0));
    CHECK(p.lds == lds_parts(p, rf));
    CHECK(p.lds <= 160 * 1024);  // the LDS of a gfx950 workgroup
    CHECK(p.nchunk == (w + (1u << p.logCW) - 1) >> p.logCW);
    const uint64_t tiles = (((uint64_t)1 << logh) >> (p.k + p.logG)) * (p.dif && !fused ? nc : 1);
    CHECK(p.grid == tiles * p.nchunk);
    CHECK(p.xcd == (tiles % 8 == 0));
    CHECK(p.logL == (p.dif ? logh - p.s0 - p.k : p.s0));
    CHECK(fused || (!p.inv_gather && !p.no_inv));
}

static void check_case(uint32_t logh, uint32_t w, uint32_t nc, bool rf, const NttKnobs& kn) {
    ctx_logh = logh, ctx_w = w, ctx_nc = nc, ctx_rf = rf;
    ctx_what = "LDE_INV";
    const std::vector<PlannedPass> inv = plan_ntt(LDE_INV, logh, w, nc, rf, kn);
    CHECK(!inv.empty());
    if (inv.empty()) return;
    uint32_t s = 0;
    for (size_t i = 0; i < inv.size(); ++i) {  // stages 0 .. logh - 1 once, in increasing order
        const PlannedPass& p = inv[i];
        check_pass(p, logh, w, nc, rf, kn);
        CHECK(!p.dif && p.s0 == s && !p.canon);
        CHECK(p.mode == (i == 0 ? PASS_INV_FIRST : PASS_INPLACE));
        CHECK(p.from_src == (i == 0));
        s += p.k;
    }
    CHECK(s == logh);
    for (int full = 0; full < 2; ++full) {
        ctx_what = full ? "LDE_FULL" : "LDE_FWD";
        const std::vector<PlannedPass> pl = plan_ntt(full ? LDE_FULL : LDE_FWD, logh, w, nc, rf, kn);
        std::vector<PlannedPass> fwd;
        size_t ninv = 0;
        for (const PlannedPass& p : pl) {
            check_pass(p, logh, w, nc, rf, kn);
            if (p.dif) {
                fwd.push_back(p);
            } else {
                CHECK(fwd.empty());  // the inverse passes come first
                ++ninv;
            }
        }
        // the inverse passes are the inverse half's, all but the last (which the fused pass runs)
        CHECK(ninv == (full ? inv.size() - 1 : 0));
        for (size_t i = 0; i < ninv && i < inv.size(); ++i)
            CHECK(pl[i].k == inv[i].k && pl[i].s0 == inv[i].s0 && pl[i].mode == inv[i].mode && !pl[i].canon);
        // the forward passes: every stage once, in the mirrored order
        CHECK(fwd.size() == inv.size());
        if (fwd.size() != inv.size()) continue;
        s = 0;
        for (size_t i = 0; i < fwd.size(); ++i) {
            const PlannedPass& p = fwd[i];
            CHECK(p.k == inv[inv.size() - 1 - i].k && p.s0 == s);
            CHECK(p.mode == (i == 0 ? PASS_INV_FWD : PASS_INPLACE));
            CHECK(p.canon == (i + 1 == fwd.size()));
            s += p.k;
        }
        CHECK(s == logh);
        // the fused pass covers the rows of the inverse's last pass
        const PlannedPass &f = fwd[0], &last = inv.back();
        CHECK(f.k == last.k && f.logL == last.logL && f.logG == last.logG && f.logCW == last.logCW);
        CHECK(f.no_inv == !full);
        CHECK(f.inv_gather == (full && inv.size() == 1));
        CHECK(f.from_src == (!full || inv.size() == 1));
    }
}

int main() {
    const uint32_t widths[] = {1, 2, 3, 5, 8, 9, 14, 47, 48, 184};
    NttKnobs alt;
    alt.kmax = 7, alt.logcw = 3, alt.twl = false;
    const NttKnobs knobs[2] = {NttKnobs{}, alt};
    for (ctx_knobs = 0; ctx_knobs < 2; ++ctx_knobs)
        for (uint32_t logh = 1; logh <= 40; ++logh)
            for (uint32_t w : widths)
                for (uint32_t nc : {1u, 8u})
                    for (int rf = 0; rf < 2; ++rf) check_case(logh, w, nc, rf != 0, knobs[ctx_knobs]);
    // the flagship shape (2^19 x 8, blowup 8): two passes of 10 and 9 stages;
    // the fused pass has k = 9, CW = 2, G = 1 and caches 511 twiddles
    ctx_what = "C1", ctx_logh = 19, ctx_w = 8, ctx_nc = 8, ctx_knobs = 0, ctx_rf = 1;
    const std::vector<PlannedPass> c1 = plan_ntt(LDE_FULL, 19, 8, 8, true, NttKnobs{});
    CHECK(c1.size() == 3);
    if (c1.size() == 3) {
        CHECK(!c1[0].dif && c1[0].mode == PASS_INV_FIRST && c1[0].k == 10 && c1[0].s0 == 0);
        CHECK(c1[1].mode == PASS_INV_FWD && c1[1].k == 9 && c1[1].logCW == 1 && c1[1].logG == 0 && c1[1].twl_n == 511);
        CHECK(c1[2].dif && c1[2].mode == PASS_INPLACE && c1[2].k == 10 && c1[2].s0 == 9 && c1[2].canon);
    }
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
