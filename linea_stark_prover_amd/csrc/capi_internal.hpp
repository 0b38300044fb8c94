// What the files of extern "C" entry points (capi.cpp, witness.cpp)
// share: the exception boundary and the host / device argument plumbing.
#pragma once
#include "prove_internal.hpp"

namespace lsp {

extern thread_local std::string g_err;  // errors without a context: lsp_last_error(NULL)

#ifdef LSP_DEBUG_BOUNDS
std::string bounds_fault_report();
#endif

// an entry point's body: exceptions become its status code, and the message
// goes to the context (or, without one, to the calling thread)
template <class F>
int guarded(lsp_ctx* ctx, F&& f) {
    try {
        f();
#ifdef LSP_DEBUG_BOUNDS
        const std::string bad = bounds_fault_report();
        if (!bad.empty()) throw LspError(LSP_E_STATE, bad);
#endif
        return LSP_OK;
    } catch (const LspError& e) {
        (ctx ? ctx->err : g_err) = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        (ctx ? ctx->err : g_err) = "host allocation failed";
        return LSP_E_OOM;
    } catch (const std::exception& e) {
        (ctx ? ctx->err : g_err) = e.what();
        return LSP_E_STATE;
    }
}

// (capi.cpp)
void need_gpu(lsp_ctx* ctx);
const Fr* dev_in(lsp_ctx* ctx, const lsp_fr* p, size_t n, int mem, const char* name);

}  // namespace lsp
