"""LDS bank-conflict model of k_ntt_rm's tile accesses.

Replays, per wave, the LDS addresses every lane of k_ntt_rm (csrc/k_ntt.hip)
issues in one pass -- the tile loads and stores, the radix-4 groups and the
radix-2 stage of tile_stages, and the reduction table of f29_reduce_qt -- and
counts the extra LDS cycles the MI355X bank rules give them
(/opt/skills/guides/MI355X_MICROARCH.md §LDS):

  ds_read_b128   4 groups of 16 lanes {0-3,12-15,20-27}, {4-11,16-19,28-31}, +32;
                 bank (a/4) mod 64
  ds_read_b32    2 groups of 32 lanes, bank (a/4) mod 32
  ds_write_b128  8 groups of 8 contiguous lanes, bank (a/4) mod 32
  ds_write_b32   2 groups of 32 lanes, bank (a/4) mod 32

An element e of the tile lives in three planes (TileLds): limbs 0-3 at
A + 16 s(e), limbs 4-7 at B + 16 s(e), limb 8 at C + 4 s(e), with s the
slot map (identity, or a swizzle).  The reduction table's entries are indexed
by a data-dependent quotient q, drawn here from a uniform range.

    python tools/lds_banks.py [--swizzle none|ntt|pad|xor] [--qrange 17]

(none: round 5's layout; ntt: the XOR map measured in round 6, docs/HISTORY.md F, + the planar q r table.)

Prints extra cycles per LDS instruction for each access site and in total,
the figure SQ_LDS_BANK_CONFLICT / SQ_INSTS_LDS measures (profiles/r05l_valu_pmc.txt:
k_ntt_rm<true,0,0> 3.90, <true,2,1> 2.17, <false,1,0> 3.08).
"""
import argparse
import random

G128 = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
        list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
G128 += [[l + 32 for l in g] for g in G128]
G32 = [list(range(0, 32)), list(range(32, 64))]
GW128 = [list(range(8 * i, 8 * i + 8)) for i in range(8)]


def extra_cycles(addrs, kind):
    """extra LDS cycles of one wave instruction; addrs[lane] = byte address or None (inactive)"""
    if kind == "r128":
        groups, mod, width = G128, 64, 4
    elif kind == "w128":
        groups, mod, width = GW128, 32, 4
    else:  # r32 / w32
        groups, mod, width = G32, 32, 1
    extra = 0
    for g in groups:
        banks = {}
        for l in g:
            a = addrs[l]
            if a is None:
                continue
            for d in range(width):
                b = (a // 4 + d) % mod
                banks.setdefault(b, set()).add(a)
        if banks:
            extra += max(len(v) for v in banks.values()) - 1
    return extra


class Model:
    def __init__(self, k, logG, logCW, swz, qrange, seed=1):
        self.k, self.logG, self.logCW = k, logG, logCW
        self.n_el = (1 << (k + logG)) << logCW
        self.swz = swz
        self.qrange = qrange
        self.rng = random.Random(seed)
        self.stats = {}

    def slot(self, e):
        if self.swz == "pad":  # one spare slot per 16 elements
            return e + (e >> 4)
        if self.swz == "xor":  # low 4 bits xor the 16-element row index's low bits
            return e ^ ((e >> 4) & 15)
        if self.swz == "ntt5":  # the first map tried (5 source bits, ~11 VALU ops)
            x = e ^ ((e >> 2) & 0x1A)
            return x ^ (0xD if (e >> 4) & 1 else 0) ^ (0xE if (e >> 7) & 1 else 0)
        if self.swz == "ntt":  # the round-6 XOR map of the NTT tile (two shift-mask terms; measured, not shipped)
            return e ^ ((e >> 1) & 8) ^ ((e >> 2) & 31)
        return e

    def planes(self):
        n = self.n_el + (self.n_el >> 4) + 1 if self.swz == "pad" else self.n_el
        return 0, 16 * n, 32 * n, 36 * n  # A, B, C, qt base (16-B aligned: n is a multiple of 4)

    def add(self, site, kind, addrs):
        s = self.stats.setdefault(site, [0, 0])
        s[0] += 1
        s[1] += extra_cycles(addrs, kind)

    def elem(self, site, lanes_e, write):
        A, B, C, _ = self.planes()
        s = [None if e is None else self.slot(e) for e in lanes_e]
        k128 = "w128" if write else "r128"
        self.add(site, k128, [None if x is None else A + 16 * x for x in s])
        self.add(site, k128, [None if x is None else B + 16 * x for x in s])
        self.add(site, "w32" if write else "r32", [None if x is None else C + 4 * x for x in s])

    def red(self, site, active):
        _, _, _, Q = self.planes()
        qs = [self.rng.randrange(self.qrange) if a else None for a in active]
        if self.swz.startswith("ntt"):  # fr29.hpp f29_qtab_init: three planes (the shipped layout)
            self.add(site + ":qt", "r128", [None if q is None else Q + 16 * q for q in qs])
            self.add(site + ":qt", "r128", [None if q is None else Q + 1024 + 16 * q for q in qs])
            self.add(site + ":qt", "r32", [None if q is None else Q + 2048 + 4 * q for q in qs])
            return
        self.add(site + ":qt", "r128", [None if q is None else Q + 48 * q for q in qs])
        self.add(site + ":qt", "r128", [None if q is None else Q + 48 * q + 16 for q in qs])
        self.add(site + ":qt", "r32", [None if q is None else Q + 48 * q + 32 for q in qs])

    def run(self, dif, use_qt, waves=4):
        k, logG, LOGCW = self.k, self.logG, self.logCW
        CW, G = 1 << LOGCW, 1 << logG
        cshift = logG + LOGCW
        for w in range(waves):
            lanes = [w * 64 + l for l in range(64)]
            # linear loads and stores (thread-strided loop)
            for it in range(self.n_el // 256):
                es = [it * 256 + t for t in lanes]
                self.elem("load", es, True)
                self.elem("store", es, False)
            j = 0
            while j + 1 < k:
                b = (k - 2 - j) if dif else j
                bmask = (1 << b) - 1
                for it in range((self.n_el >> 2) // 256 or 1):
                    e0s = []
                    for t in lanes:
                        qd = t + it * 256
                        if qd >= (self.n_el >> 2):
                            e0s.append(None)
                            continue
                        c = qd & (CW - 1)
                        pg = qd >> LOGCW
                        g, pp = pg & (G - 1), pg >> logG
                        t0 = ((pp & ~bmask) << 2) | (pp & bmask)
                        e0s.append((t0 << cshift) + (g << LOGCW) + c)
                    de = (1 << b) << cshift
                    for m in range(4):
                        self.elem(f"r4 b={b}", [None if e is None else e + m * de for e in e0s], False)
                    if use_qt:
                        for _ in range(2):
                            self.red(f"r4 b={b}", [e is not None for e in e0s])
                    for m in range(4):
                        self.elem(f"r4 b={b}", [None if e is None else e + m * de for e in e0s], True)
                j += 2
            if j < k:
                logd = 0 if dif else j
                dmask = (1 << logd) - 1
                for it in range((self.n_el >> 1) // 256):
                    a0s = []
                    for t in lanes:
                        bf = t + it * 256
                        c = bf & (CW - 1)
                        pg = bf >> LOGCW
                        g, pp = pg & (G - 1), pg >> logG
                        t0 = ((pp >> logd) << (logd + 1)) | (pp & dmask)
                        a0s.append((t0 << cshift) + (g << LOGCW) + c)
                    d = (1 << logd) << cshift
                    for m in range(2):
                        self.elem(f"r2 d={logd}", [a + m * d for a in a0s], False)
                    if use_qt:
                        self.red(f"r2 d={logd}", [True] * 64)
                    for m in range(2):
                        self.elem(f"r2 d={logd}", [a + m * d for a in a0s], True)

    def report(self, title):
        tot_i = sum(v[0] for v in self.stats.values())
        tot_x = sum(v[1] for v in self.stats.values())
        print(f"{title}: {tot_x / tot_i:.2f} extra cycles per LDS instruction ({tot_i} instructions)")
        for site, (n, x) in sorted(self.stats.items()):
            print(f"   {site:16s} {n:6d} instr  {x / n:5.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--swizzle", default="none")
    ap.add_argument("--qrange", type=int, default=17)
    a = ap.parse_args()
    # the three passes of a 2^19 x 8 LDE (plan_ntt: ks = [10, 9])
    for name, k, logG, logCW, dif, qt in (("k_ntt_rm<false,1,0> (inverse first, k=10)", 10, 0, 0, False, True),
                                          ("k_ntt_rm<true,2,1> fused (k=9, CW=2), forward stages", 9, 0, 1, True, False),
                                          ("k_ntt_rm<true,0,0> in place (k=10)", 10, 0, 0, True, True)):
        m = Model(k, logG, logCW, a.swizzle, a.qrange)
        m.run(dif, qt)
        m.report(name)


if __name__ == "__main__":
    main()
