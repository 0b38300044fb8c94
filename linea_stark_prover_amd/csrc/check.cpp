// p3-uni-stark check_constraints (lsp_check_constraints): the device path
// around k_check.hip and its host twin, a plain loop over the rows with
// Air::eval.  Both fill the same report, field for field.
#include <algorithm>

#include "prove_internal.hpp"

namespace lsp {

namespace {
void summarise(CheckReport& r) {
    r.s.violations = 0;
    r.s.first_row = UINT64_MAX;
    r.s.first_constraint = UINT32_MAX;
    for (uint32_t j = 0; j < r.s.ncons; ++j) {
        r.s.violations += r.counts[j];
        if (r.first_rows[j] < r.s.first_row) {  // the lowest j among equal rows: strict
            r.s.first_row = r.first_rows[j];
            r.s.first_constraint = j;
        }
    }
}

void check_shape(size_t h, size_t w, const Air& air, size_t npub, const Fr* prep, size_t wp) {
    LSP_REQUIRE((prep != nullptr) == (wp != 0), LSP_E_ARG, "a preprocessed matrix needs a pointer and a width");
    air.require_fits(w, npub, wp);
    (void)log2_exact(h);
}
}  // namespace

CheckReport check_constraints_host(const Fr* trace, size_t h, size_t w, const Air& air, const Fr* pub, size_t npub,
                                   size_t cap, const Fr* prep, size_t wp) {
    check_shape(h, w, air, npub, prep, wp);
    CheckReport r;
    const uint32_t nc = air.num_constraints();
    r.s = lsp_check_summary{0, 0, UINT64_MAX, UINT32_MAX, nc};
    r.counts.assign(nc, 0);
    r.first_rows.assign(nc, UINT64_MAX);
    const Fr one = fr_one(), zero = fr_zero();
    std::vector<Fr> vals(nc);
    for (size_t i = 0; i < h; ++i) {
        const Fr* loc = trace + i * w;
        const size_t in = i + 1 == h ? 0 : i + 1;
        const Fr* nxt = trace + in * w;
        const bool last = i + 1 == h;
        uint32_t j = 0;
        bool any = false;
        air.eval(loc, nxt, pub, i == 0 ? one : zero, last ? one : zero, last ? zero : one,
                 [&](const Fr& x) {
                     vals[j] = x;
                     if (!fr_is_zero(x)) {
                         any = true;
                         ++r.counts[j];
                         r.first_rows[j] = std::min<uint64_t>(r.first_rows[j], i);
                     }
                     ++j;
                 },
                 prep ? prep + i * wp : nullptr, prep ? prep + in * wp : nullptr);
        if (!any) continue;
        ++r.s.failed_rows;
        for (uint32_t k = 0; k < nc && r.list.size() < cap; ++k)
            if (!fr_is_zero(vals[k])) r.list.push_back(lsp_violation{i, k, 0, from_fr(vals[k])});
    }
    summarise(r);
    return r;
}

CheckReport check_constraints_device(lsp_ctx* ctx, const Fr* d_trace, size_t h, size_t w, const Air& air,
                                     const Fr* pub, size_t npub, size_t cap, const Fr* d_prep, size_t wp) {
    check_shape(h, w, air, npub, d_prep, wp);
    CheckReport r;
    const uint32_t nc = air.num_constraints();
    r.s = lsp_check_summary{0, 0, UINT64_MAX, UINT32_MAX, nc};
    const size_t nwords = (h + 63) / 64;
    uint64_t* mask = (uint64_t*)ctx->buf("chk_mask", nwords * sizeof(uint64_t));
    uint64_t* cnt = (uint64_t*)ctx->buf("chk_count", 2 * (size_t)nc * sizeof(uint64_t));
    int32_t* dair = (int32_t*)ctx->buf("chk_air", air.dev.size() * sizeof(int32_t));
    LSP_HIP(hipMemcpyAsync(dair, air.dev.data(), air.dev.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                           ctx->stream));
    LSP_HIP(hipMemsetAsync(mask, 0, nwords * sizeof(uint64_t), ctx->stream));
    LSP_HIP(hipMemsetAsync(cnt, 0, (size_t)nc * sizeof(uint64_t), ctx->stream));
    LSP_HIP(hipMemsetAsync(cnt + nc, 0xff, (size_t)nc * sizeof(uint64_t), ctx->stream));
    CheckArgs a;
    a.trace = d_trace;
    a.h = h;
    a.w = (uint32_t)w;
    a.air = dair;
    a.ncons = nc;
    a.pub_alpha = pub[0];
    a.pub_delta = pub[1];
    if (air.has_prog) {  // (pub outlives the copy: the ctx->sync() below)
        Fr* dpub = ctx->fbuf("chk_pub", npub);
        LSP_HIP(hipMemcpyAsync(dpub, pub, npub * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        a.pub = dpub;
        a.npub = (uint32_t)npub;
        a.prog = 1;
        a.prog_slots = air.prog_slots;
        a.prep = d_prep;
        a.wp = (uint32_t)wp;
    }
    a.row_mask = mask;
    a.count = cnt;
    a.first_row = cnt + nc;
    LSP_HIP(launch_check(a, ctx->stream));
    std::vector<uint64_t> hm(nwords), hc(2 * (size_t)nc);
    LSP_HIP(hipMemcpyAsync(hm.data(), mask, nwords * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    LSP_HIP(hipMemcpyAsync(hc.data(), cnt, hc.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    r.counts.assign(hc.begin(), hc.begin() + nc);
    r.first_rows.assign(hc.begin() + nc, hc.end());
    for (uint64_t m : hm) r.s.failed_rows += (uint64_t)__builtin_popcountll(m);
    summarise(r);
    // the detail records: every failing row holds at least one violation, so
    // the first `cap` violations lie in the first `cap` failing rows
    const size_t nr = (size_t)std::min<uint64_t>(cap, r.s.failed_rows);
    if (!nr) return r;
    std::vector<uint64_t> rows;
    rows.reserve(nr);
    for (size_t k = 0; k < nwords && rows.size() < nr; ++k)
        for (uint64_t m = hm[k]; m && rows.size() < nr; m &= m - 1)
            rows.push_back(64 * (uint64_t)k + (uint64_t)__builtin_ctzll(m));
    uint64_t* drows = (uint64_t*)ctx->buf("chk_rows", nr * sizeof(uint64_t));
    Fr* dvals = ctx->fbuf("chk_vals", nr * nc);
    LSP_HIP(hipMemcpyAsync(drows, rows.data(), nr * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    a.rows = drows;
    a.nrows = (uint32_t)nr;
    a.vals = dvals;
    LSP_HIP(launch_check_rows(a, ctx->stream));
    std::vector<Fr> vals(nr * nc);
    LSP_HIP(hipMemcpyAsync(vals.data(), dvals, vals.size() * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    for (size_t k = 0; k < nr && r.list.size() < cap; ++k)
        for (uint32_t j = 0; j < nc && r.list.size() < cap; ++j)
            if (!fr_is_zero(vals[k * nc + j])) r.list.push_back(lsp_violation{rows[k], j, 0, from_fr(vals[k * nc + j])});
    return r;
}

static const char* kind_name(int32_t kind) {
    switch (kind) {
        case LSP_CONSTRAINT_B_INVERSE: return "b_inverse";
        case LSP_CONSTRAINT_A_INVERSE: return "a_inverse";
        case LSP_CONSTRAINT_FIRST_ROW: return "first_row";
        case LSP_CONSTRAINT_TRANSITION: return "transition";
        case LSP_CONSTRAINT_PROGRAM: return "program assert";
        default: return "last_row";
    }
}

std::string check_failure_message(const Air& air, const CheckReport& r) {
    const Air::ConsInfo ci = air.constraint_info(r.s.first_constraint);
    std::string m = "constraints had nonzero value on row " + std::to_string(r.s.first_row) + ": constraint " +
                    std::to_string(r.s.first_constraint) + " (config " + std::to_string(ci.config) + ", " +
                    kind_name(ci.kind);
    if (ci.table >= 0) m += ", table " + std::to_string(ci.table);
    return m + "); " + std::to_string(r.s.failed_rows) + " rows fail";
}

}  // namespace lsp
