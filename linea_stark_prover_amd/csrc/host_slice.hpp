// The host slice of a big Merkle tree: while the GPU
// hashes the leaves and the wide levels, the host pool -- idle for those
// milliseconds -- hashes the LAST aligned subtree of n >> log_frac leaves,
// leaves [n - (n >> log_frac), n).  The GPU's share of every layer is then a
// prefix: each level stays one launch, with a smaller count.  The two halves
// meet in the layer of `join` digests the host's tree top starts from.
//
// Plain C++, no HIP: tests/host_slice_check.cpp builds it alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace lsp {

constexpr size_t HOST_SLICE_MIN_LEAVES = (size_t)1 << 21;  // smaller trees: the copy and the hand-off outweigh the slice
// the host's predicted time may be at most this part of the GPU's: a late host
// stalls the GPU at the join, an early one only idles as before
constexpr double HOST_SLICE_MARGIN = 0.85;
constexpr uint32_t HOST_SLICE_LOG_FRAC_FIRST = 5, HOST_SLICE_LOG_FRAC_LAST = 7;  // 1/32, 1/64, 1/128

struct HostSliceIn {
    size_t leaves = 0;          // a power of two
    size_t perms_per_leaf = 1;  // permutations of a leaf's row sponge
    size_t join = 0;            // digests of the layer where the halves meet (a power of two, < leaves); 0: none
    double host_perm_s = 0;     // permutations per second: the whole host pool's,
    double gpu_perm_s = 0;      // the GPU's
    bool shared = false;        // a communicator, several proofs in flight, several ranks on the host: off
    int forced = -1;            // LSP_HOST_SLICE: -1 not set, 0 off, k: log_frac = k whatever the size and the rates
};

struct HostSlice {
    uint32_t log_frac = 0;  // 0: no slice
    explicit operator bool() const { return log_frac != 0; }
    // of a layer of `len` digests (or of the leaves): the host's last part and the GPU's prefix
    size_t slice(size_t len) const { return log_frac ? len >> log_frac : 0; }
    size_t prefix(size_t len) const { return len - slice(len); }
};

// permutations below the join layer in the subtree over `leaves` leaves that
// ends in `roots` digests of it: the leaf sponges and the compressions
inline double slice_perms(size_t leaves, size_t perms_per_leaf, size_t roots) {
    return (double)leaves * (double)perms_per_leaf + (double)(leaves - roots);
}

inline bool host_slice_fits(const HostSliceIn& in, uint32_t log_frac) {
    if (log_frac == 0 || log_frac >= 8 * sizeof(size_t)) return false;
    if (in.join == 0 || (in.join & (in.join - 1)) || in.leaves <= in.join || (in.leaves & (in.leaves - 1))) return false;
    return (in.join >> log_frac) >= 1;  // the slice holds whole digests of the join layer
}

inline HostSlice plan_host_slice(const HostSliceIn& in) {
    if (in.forced == 0) return {};
    if (in.forced > 0) return host_slice_fits(in, (uint32_t)in.forced) ? HostSlice{(uint32_t)in.forced} : HostSlice{};
    if (in.shared || in.leaves < HOST_SLICE_MIN_LEAVES || !(in.host_perm_s > 0) || !(in.gpu_perm_s > 0)) return {};
    for (uint32_t lf = HOST_SLICE_LOG_FRAC_FIRST; lf <= HOST_SLICE_LOG_FRAC_LAST; ++lf) {
        if (!host_slice_fits(in, lf)) break;
        const HostSlice s{lf};
        const double host_s = slice_perms(s.slice(in.leaves), in.perms_per_leaf, s.slice(in.join)) / in.host_perm_s;
        const double gpu_s = slice_perms(s.prefix(in.leaves), in.perms_per_leaf, s.prefix(in.join)) / in.gpu_perm_s;
        if (host_s <= HOST_SLICE_MARGIN * gpu_s) return s;
    }
    return {};
}

}  // namespace lsp
