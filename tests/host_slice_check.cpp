// The host slice's plan (csrc/host_slice.hpp), checked on the host alone:
// built and run by tests/test_host_slice_plan.py.  Prints one line per broken
// property and exits nonzero if there is any.
#include <cstdio>

#include "host_slice.hpp"

using namespace lsp;

static int failures = 0;
static uint32_t c_logn, c_lf;
static const char* c_what = "";

#define CHECK(cond)                                                                               \
    do {                                                                                          \
        if (!(cond) && ++failures <= 40)                                                          \
            std::printf("FAIL %s log n=%u log_frac=%u: %s\n", c_what, c_logn, c_lf, #cond);       \
    } while (0)

// rates at which 1/32 takes exactly `ratio` of the GPU's time (host time /
// GPU time = gpu rate * slice perms / (host rate * prefix perms))
static HostSliceIn big(uint32_t logn, double ratio_at_32) {
    HostSliceIn in;
    in.leaves = (size_t)1 << logn;
    in.perms_per_leaf = 4;
    in.join = 1024;
    in.host_perm_s = 29e6;
    const HostSlice s{5};
    in.gpu_perm_s = ratio_at_32 * in.host_perm_s * slice_perms(s.prefix(in.leaves), 4, s.prefix(in.join)) /
                    slice_perms(s.slice(in.leaves), 4, s.slice(in.join));
    return in;
}

int main() {
    // ---- below 2^21 leaves: no slice, whatever the rates; from 2^21 on, 1/32 with a fast host
    c_what = "size threshold";
    for (c_logn = 6; c_logn <= 26; ++c_logn) {
        c_lf = 0;
        HostSliceIn in = big(c_logn, 0.5);
        if (in.leaves <= in.join) in.join = in.leaves / 2;
        const HostSlice s = plan_host_slice(in);
        if (c_logn < 21)
            CHECK(!s && s.log_frac == 0);
        else
            CHECK(s.log_frac == 5);
        in.forced = 0;  // the knob's 0 switches it off at every size
        CHECK(!plan_host_slice(in));
        in.forced = -1;
        in.shared = true;  // as do a communicator, other proofs, other ranks
        CHECK(!plan_host_slice(in));
    }
    // ---- the 0.85 rule: a smaller fraction, then none
    c_what = "0.85 rule";
    c_logn = 22;
    c_lf = 0;
    CHECK(plan_host_slice(big(22, 0.84)).log_frac == 5);
    CHECK(plan_host_slice(big(22, 0.86)).log_frac == 6);
    CHECK(plan_host_slice(big(22, 1.0)).log_frac == 6);
    CHECK(plan_host_slice(big(22, 1.6)).log_frac == 6);   // 1/64 takes a little over half of 1/32's ratio
    CHECK(plan_host_slice(big(22, 1.75)).log_frac == 7);
    CHECK(plan_host_slice(big(22, 3.2)).log_frac == 7);
    CHECK(plan_host_slice(big(22, 3.6)).log_frac == 0);
    CHECK(plan_host_slice(big(22, 100.0)).log_frac == 0);
    {
        HostSliceIn in = big(22, 0.5);  // rates never measured: none
        in.host_perm_s = 0;
        CHECK(!plan_host_slice(in));
        in = big(22, 0.5);
        in.gpu_perm_s = 0;
        CHECK(!plan_host_slice(in));
        in = big(22, 0.5);  // no join layer (the tree top is not on the host): none
        in.join = 0;
        CHECK(!plan_host_slice(in));
    }
    // ---- forced: every size, the shared host included; aligned, last, and the counts add up
    c_what = "forced";
    for (c_logn = 6; c_logn <= 26; ++c_logn)
        for (c_lf = 1; c_lf <= 27; ++c_lf)
            for (uint32_t logj = 0; logj < c_logn; ++logj) {
                HostSliceIn in;
                in.leaves = (size_t)1 << c_logn;
                in.join = (size_t)1 << logj;
                in.shared = true;
                in.forced = (int)c_lf;
                const HostSlice s = plan_host_slice(in);
                if (c_lf > logj) {  // less than one digest of the join layer: no slice
                    CHECK(!s);
                    continue;
                }
                CHECK(s.log_frac == c_lf);
                // every layer from the leaves to the join: prefix + slice = the layer, the slice is
                // the last aligned subtree's part of it, and the prefix of a layer is what the prefix
                // of the layer above needs
                for (size_t len = in.leaves; len >= in.join; len /= 2) {
                    const size_t sl = s.slice(len), pre = s.prefix(len);
                    CHECK(sl >= 1 && pre + sl == len);
                    CHECK(sl == len >> c_lf && (sl & (sl - 1)) == 0);
                    CHECK(pre % sl == 0);  // aligned: the slice starts at a multiple of its size
                    CHECK(pre / sl == ((size_t)1 << c_lf) - 1);  // and is the last of the 2^log_frac subtrees
                    if (len > in.join) CHECK(pre == 2 * s.prefix(len / 2) && sl == 2 * s.slice(len / 2));
                }
                // the permutations of both halves are the tree's
                const double all = slice_perms(in.leaves, 3, in.join);
                CHECK(slice_perms(s.slice(in.leaves), 3, s.slice(in.join)) +
                          slice_perms(s.prefix(in.leaves), 3, s.prefix(in.join)) == all);
            }
    // ---- the fractions the rule may pick are 1/32, 1/64, 1/128 only, and need the join layer to hold them
    c_what = "join too small";
    c_logn = 22;
    {
        HostSliceIn in = big(22, 0.5);
        in.join = 16;  // 16 >> 5 = 0
        CHECK(!plan_host_slice(in));
        in.join = 32;
        CHECK(plan_host_slice(in).log_frac == 5);
        in = big(22, 1.0);
        in.join = 32;  // 1/64 would fit the rule, not the layer
        CHECK(!plan_host_slice(in));
        in.join = 48;  // not a power of two
        CHECK(!plan_host_slice(in));
    }
    std::printf("%d failure(s)\n", failures);
    return failures != 0;
}
