// The one codec of the wire formats (proof.cpp "LSPPRF02" /
// "LSPPRF03", pcs.cpp "LSPPCS01", read again by verify.cpp): little-endian
// 32-bit words and field elements as 32-byte little-endian canonical integers.
// Host code over untrusted bytes (tools/sanitize builds it under ASan / UBSan).
#pragma once
#include <cstring>
#include <vector>

#include "host.hpp"

namespace lsp {

// writes in one pass into a buffer the caller sized up front
struct Writer {
    uint8_t* p;
    void u32(uint32_t x) {
        for (int i = 0; i < 4; ++i) *p++ = (uint8_t)(x >> (8 * i));
    }
    void fr(const Fr& x) {
        // Montgomery form -> integer: one Montgomery reduction (a product by 1
        // without the product rows) on the 4 x 64-bit host arithmetic
        const Fr c = hp64::to_canonical(hp64::redc(hp64::from(x)));
        std::memcpy(p, c.v, 32);  // 32-bit words little-endian (x86-64 host)
        p += 32;
    }
    void frs(const std::vector<Fr>& v) {
        for (auto& x : v) fr(x);
    }
    void path(const std::vector<Fr>& v) {  // a counted vector
        u32((uint32_t)v.size());
        frs(v);
    }
};

// bounds-checked reader: every overrun or non-canonical element sets `bad`,
// and a bad reader reads nothing more
struct Reader {
    const uint8_t* b;
    size_t n, off = 0;
    bool bad = false;
    size_t left() const { return n - off; }
    uint32_t u32() {
        if (bad || left() < 4) {
            bad = true;
            return 0;
        }
        uint32_t x = 0;
        for (int i = 0; i < 4; ++i) x |= (uint32_t)b[off + i] << (8 * i);
        off += 4;
        return x;
    }
    Fr fr() {
        Fr c = fr_zero();
        if (bad || left() < 32) {
            bad = true;
            return c;
        }
        for (int i = 0; i < 8; ++i) {
            uint32_t x = 0;
            for (int k = 0; k < 4; ++k) x |= (uint32_t)b[off + 4 * i + k] << (8 * k);
            c.v[i] = x;
        }
        off += 32;
        if (!fr_words_lt_mod(c)) {
            bad = true;
            return fr_zero();
        }
        return fr_from_canonical(c);
    }
    // cnt elements, refusing counts the remaining bytes cannot hold (nothing is sized before that)
    void frs(std::vector<Fr>& v, uint64_t cnt) {
        if (bad || cnt > left() / 32) {
            bad = true;
            return;
        }
        v.resize((size_t)cnt);
        for (Fr& x : v) x = fr();
    }
};

}  // namespace lsp
