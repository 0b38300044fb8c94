// The pass plan of a coset LDE (k_ntt.hip): which passes run, in which order,
// and each one's tile geometry, grid and LDS bytes.  Plain C++ with no HIP
// types, so the host compiler alone builds it (tests/test_ntt_plan.py).
//
// A pass fuses k radix-2 stages on a tile of 2^k positions x 2^logG adjacent
// row groups x 2^logCW adjacent columns, at most NTT_MAX_EL elements (36 KiB
// of LDS), so every radix-4 group gives each of the 256 threads one quad.  Up
// to k = 10 stages per pass with one column per tile (2^19 points in 2 passes
// instead of 3: fewer HBM round trips); a pass with fewer stages takes the
// widest column chunk that still fits (k = 9: CW = 2, ..., k <= 7: CW = 8),
// and the narrow row accesses are merged in L2 by the XCD-aware tile order.
// The inverse runs passes ks[0], ..., ks[np-1] (DIT, stages in increasing
// order), the forward ks[np-1], ..., ks[0] (DIF), so the forward's first pass
// covers the rows of the inverse's last and the two run as one (PASS_INV_FWD).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace lsp {

// the passes of an LDE (LDE_FULL), of its inverse half only (LDE_INV: scratch
// <- h * coefficients) or of its forward half only (LDE_FWD: from h *
// coefficients at the source)
enum LdeWhat { LDE_FULL = 0, LDE_INV = 1, LDE_FWD = 2 };
// PASS_INV_FIRST gathers the caller's rows bit-reversed; PASS_INV_FWD is the
// inverse's last pass fused with the forward's first, looping over the cosets
enum PassMode : int { PASS_INPLACE = 0, PASS_INV_FIRST = 1, PASS_INV_FWD = 2 };

constexpr uint32_t NTT_THREADS = 256;
constexpr uint32_t NTT_MAX_EL = 1024;       // 2^k x G x CW
constexpr uint32_t NTT_TWL_MAX = 512;       // forward twiddles the fused pass caches in LDS (2 workgroups per CU)
constexpr size_t NTT_EL_BYTES = 36;         // an F29 (nine 29-bit limbs)
constexpr size_t NTT_TWL_BYTES = 48;        // a cached twiddle (TwlLds: a padded slot)
constexpr size_t NTT_QTAB_BYTES = 64 * 48;  // the reduction table the plain passes keep after the tile (f29_qtab_init)

// LSP_NTT_KMAX, LSP_NTT_LOGCW (-1: by width), LSP_NTT_TWL
struct NttKnobs {
    uint32_t kmax = 10;
    int logcw = -1;
    bool twl = true;
};

struct PlannedPass {
    bool dif;  // a forward pass (on the output blocks); else an inverse pass (on the scratch)
    PassMode mode;
    uint32_t k, s0;    // stages s0 .. s0 + k - 1
    uint32_t logL;     // log2 of the row stride between a tile's positions
    uint32_t logG, logCW, nchunk;
    uint64_t grid;     // workgroups: tiles x chunks (x cosets, except in the fused pass)
    size_t lds;        // dynamic LDS bytes
    uint32_t twl_n;    // the fused pass: forward twiddles cached in LDS (0: read from the table)
    bool xcd, canon;   // XCD-aware tile order; canonical output (the transform's last pass)
    bool from_src;     // reads the caller's source (else the scratch)
    bool inv_gather;   // the fused pass: the inverse has only this pass (source rows gathered bit-reversed)
    bool no_inv;       // the fused pass: the source holds coefficients (LDE_FWD)
};

// the stages of each pass: as few passes as kmax allows, as even as possible
inline std::vector<uint32_t> plan_stages(uint32_t logh, uint32_t kmax) {
    if (logh <= kmax) return {logh};
    const uint32_t P = (logh + kmax - 1) / kmax;
    std::vector<uint32_t> ks(P);
    for (uint32_t q = 0; q < P; ++q) ks[q] = logh / P + (q < logh % P ? 1 : 0);
    return ks;
}

// The ordered passes of `what` on 2^logh rows x w columns and ncosets output
// blocks (logh >= 1, w >= 1).  row_factors: the fused pass keeps one factor per
// tile row in LDS (a twist shared by every column, or the chained twist).
inline std::vector<PlannedPass> plan_ntt(LdeWhat what, uint32_t logh, size_t w, uint32_t ncosets, bool row_factors,
                                         const NttKnobs& kn) {
    uint32_t logCWmax = 0;  // the power of two >= min(w, 8)
    while ((1u << logCWmax) < w && logCWmax < 3) ++logCWmax;
    // minimum log2 column chunk (bounds k).  Narrow chunks rely on the XCD's L2
    // holding a tile's rows until all its chunks have read them; from ~48
    // columns (1.5 MiB per 1024-row tile) passes of whole 256-byte row segments
    // win (profiles/r02u_lde_logcw.txt)
    const uint32_t logcw_min = kn.logcw >= 0 ? (uint32_t)std::min(3, kn.logcw) : (w >= 48 ? 1u : 0u);
    const uint32_t kmax = std::min(std::min(10u, std::max(1u, kn.kmax)), 10 - std::min(logCWmax, logcw_min));
    const std::vector<uint32_t> ks = plan_stages(logh, kmax);
    const uint32_t np = (uint32_t)ks.size();
    std::vector<PlannedPass> plan;
    auto add = [&](bool dif, PassMode mode, uint32_t k, uint32_t s0, bool canon) {
        const bool fused = mode == PASS_INV_FWD;
        PlannedPass p{};
        p.dif = dif;
        p.mode = mode;
        p.k = k;
        p.s0 = s0;
        p.logL = dif ? logh - s0 - k : s0;
        p.logCW = std::min(logCWmax, 10 - k);  // the widest chunk the tile allows at this k
        p.logG = std::min(logh - k, 10 - k - p.logCW);
        p.nchunk = (uint32_t)((w + (1u << p.logCW) - 1) >> p.logCW);
        const uint64_t tiles = ((uint64_t)1 << logh) >> (k + p.logG);
        // the fused pass loops over the cosets inside each workgroup
        p.grid = (uint64_t)(dif && !fused ? ncosets : 1) * tiles * p.nchunk;
        const size_t rows = (size_t)1 << (k + p.logG);
        p.lds = ((rows << p.logCW) + (fused && row_factors ? rows : 0)) * NTT_EL_BYTES;
        const size_t twl_n = ((size_t)1 << p.logG) * (((size_t)1 << k) - 1);
        p.twl_n = fused && kn.twl && twl_n <= NTT_TWL_MAX ? (uint32_t)twl_n : 0u;
        if (p.twl_n) p.lds = ((p.lds + 15) & ~(size_t)15) + p.twl_n * NTT_TWL_BYTES;
        if (!fused) p.lds += NTT_QTAB_BYTES;
        p.xcd = (p.grid / p.nchunk) % 8 == 0;
        p.canon = canon;
        p.from_src = mode == PASS_INV_FIRST || (fused && (np == 1 || what == LDE_FWD));
        p.inv_gather = fused && np == 1 && what == LDE_FULL;
        p.no_inv = fused && what == LDE_FWD;
        plan.push_back(p);
    };
    uint32_t s0 = 0;
    // the inverse passes; an LDE's last one runs inside the fused pass
    for (uint32_t q = 0; what != LDE_FWD && q + (what == LDE_FULL ? 1 : 0) < np; ++q) {
        add(false, q == 0 ? PASS_INV_FIRST : PASS_INPLACE, ks[q], s0, false);
        s0 += ks[q];
    }
    if (what == LDE_INV) return plan;
    add(true, PASS_INV_FWD, ks[np - 1], 0, np == 1);
    s0 = ks[np - 1];
    for (uint32_t q = 1; q < np; ++q) {  // the remaining forward passes
        add(true, PASS_INPLACE, ks[np - 1 - q], s0, q + 1 == np);
        s0 += ks[np - 1 - q];
    }
    return plan;
}

}  // namespace lsp
