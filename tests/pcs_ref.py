"""A big-integer TwoAdicFriPcs over batches of unequal heights (DESIGN.md
section 3, U15): the reference of tests/test_pcs.py (CPU) and
tests/test_gpu_pcs.py.  No tests in this module.

Built only from oracle.pyoracle's coset_lde_batch, interpolate_coset,
inverse_denominators, open_reduce, fold_vector, fold_row, HashChallenger and
idft (with its plain Merkle tree for the FRI rounds), from
tests/mixed_mmcs_ref.py's mixed-height tree, and an LSPPCS01 serializer; with
its own `verify`.  Matrices are lists of rows of canonical values.
"""
import os
import struct
import sys
from dataclasses import dataclass, field
from typing import List

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import mixed_mmcs_ref as MM  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

P = O.P


@dataclass
class Committed:
    """one batch: the matrices' LDEs (bit-reversed, on GEN * H_N) under one mixed-height tree"""
    ldes: List[List[List[int]]]
    tree: MM.Tree

    @property
    def root(self):
        return self.tree.root

    def dims(self, fri):
        """[(height, width)] as given to commit"""
        return [(len(m) >> fri.log_blowup, len(m[0])) for m in self.ldes]


def commit(mats, shifts, pp, fri) -> Committed:
    shifts = shifts or [1] * len(mats)
    ldes = [O.coset_lde_batch(m, fri.log_blowup, O.GENERATOR * O.inv(s) % P) for m, s in zip(mats, shifts)]
    return Committed(ldes, MM.commit(ldes, pp))


@dataclass
class Proof:
    shape: list            # [batch][matrix] -> (width, points)
    ys: list               # [batch][matrix][point][column]
    roots: List[int]
    final_poly: List[int]
    pow_witness: int
    # per query: ([(rows per matrix, path) per batch], [(sibling, path) per round])
    queries: list = field(default_factory=list)


def open(coms, rounds, ch, pp, fri, log=None):
    """coms: [Committed]; rounds[b][j]: the points of matrix j of batch b (may be
    empty).  Returns (ys, Proof).  log (optional) receives alpha, ro (by LDE
    height), betas."""
    lb = fri.log_blowup
    log = log if log is not None else {}
    ys = [[[O.interpolate_coset(lde[:len(lde) >> lb], O.GENERATOR, z) for z in zs] for lde, zs in zip(c.ldes, pts)]
          for c, pts in zip(coms, rounds)]
    if fri.observe_opened_values:  # U7: the nesting order
        ch.observe_slice([v for b in ys for m in b for p in m for v in p])
    alpha = ch.sample()
    ro, off, invd = {}, {}, {}
    for c, pts, yb in zip(coms, rounds, ys):
        for lde, zs, ym in zip(c.ldes, pts, yb):
            if not zs:
                continue
            N = len(lde)
            ro.setdefault(N, [0] * N)
            for z in zs:  # once per (height, distinct point)
                if (N, z) not in invd:
                    invd[N, z] = O.inverse_denominators(O.log2_strict(N), O.GENERATOR, [z])[0]
            off[N] = O.open_reduce(lde, [invd[N, z] for z in zs], ym, alpha, off.get(N, 1), ro[N])
    log.update(alpha=alpha, ro=ro)

    nmax = max(len(lde) for c in coms for lde in c.ldes)
    folded = list(ro[nmax])
    trees, betas = [], []
    while len(folded) > 1 << (lb + fri.log_final_poly_len):
        tr = O.merkle_commit([[[folded[2 * i], folded[2 * i + 1]] for i in range(len(folded) // 2)]], pp)
        ch.observe(tr.root)
        betas.append(ch.sample())
        trees.append(tr)
        folded = O.fold_vector(folded, betas[-1])
        if len(folded) in ro:  # the roll-in: plain addition
            folded = [(a + b) % P for a, b in zip(folded, ro[len(folded)])]
    coeffs = O.idft(O.reverse_slice_index_bits(folded))
    flen = 1 << fri.log_final_poly_len
    assert all(c == 0 for c in coeffs[flen:]), "final poly degree too high"
    final_poly = coeffs[:flen]
    if fri.observe_final_poly:
        ch.observe_slice(final_poly)
    log["betas"] = betas
    pow_w = ch.grind(fri.proof_of_work_bits)

    lmax = O.log2_strict(nmax)
    queries = []
    for _ in range(fri.num_queries):
        idx = ch.sample_bits(lmax)
        inputs = [MM.open(c.tree, idx >> (lmax - O.log2_strict(len(c.tree.layers[0])))) for c in coms]
        steps = []
        for r, tr in enumerate(trees):
            ii = idx >> r
            rows, path = O.merkle_open(tr, ii >> 1)
            steps.append((rows[0][(ii ^ 1) & 1], path))
        queries.append((inputs, steps))
    shape = [[(len(lde[0]), len(zs)) for lde, zs in zip(c.ldes, pts)] for c, pts in zip(coms, rounds)]
    return ys, Proof(shape, ys, [t.root for t in trees], final_poly, pow_w, queries)


def verify(commits, dims, rounds, proof: Proof, ch, pp, fri) -> bool:
    """commits[b]: batch b's root; dims[b][j] = (height, width) as given to
    commit; rounds[b][j]: the points.  Restated from U15, not from `open`."""
    lb = fri.log_blowup
    shape = [[(w, len(zs)) for (_, w), zs in zip(d, pts)] for d, pts in zip(dims, rounds)]
    if proof.shape != shape or len(proof.ys) != len(shape):
        return False
    heights = [[h << lb for h, _ in d] for d in dims]
    lmax = O.log2_strict(max(n for hs in heights for n in hs))
    nr = lmax - lb - fri.log_final_poly_len
    if len(proof.roots) != nr or len(proof.final_poly) != 1 << fri.log_final_poly_len:
        return False
    if len(proof.queries) != fri.num_queries:
        return False
    if fri.observe_opened_values:
        ch.observe_slice([v for b in proof.ys for m in b for p in m for v in p])
    alpha = ch.sample()
    betas = []
    for root in proof.roots:
        ch.observe(root)
        betas.append(ch.sample())
    if fri.observe_final_poly:
        ch.observe_slice(proof.final_poly)
    if not ch.check_witness(fri.proof_of_work_bits, proof.pow_witness):
        return False
    for inputs, steps in proof.queries:
        idx = ch.sample_bits(lmax)
        if len(inputs) != len(commits) or len(steps) != nr:
            return False
        ro, k = {}, {}
        for root, hs, d, pts, yb, (rows, path) in zip(commits, heights, dims, rounds, proof.ys, inputs):
            lbatch = O.log2_strict(max(hs))
            if len(rows) != len(hs) or any(len(r) != w for r, (_, w) in zip(rows, d)):
                return False
            if not MM.verify(root, hs, idx >> (lmax - lbatch), rows, path, pp):
                return False
            for N, (_, w), zs, ym, row in zip(hs, d, pts, yb, rows):
                logn = O.log2_strict(N)
                x = O.GENERATOR * pow(O.two_adic_generator(logn), O.bitrev(idx >> (lmax - logn), logn), P) % P
                for z, yz in zip(zs, ym):
                    kk = k.get(N, 0)
                    num = sum(pow(alpha, c, P) * (yz[c] - row[c]) for c in range(w)) % P
                    ro[N] = (ro.get(N, 0) + pow(alpha, kk, P) * num % P * O.inv(z - x)) % P
                    k[N] = kk + w
        folded, index = 0, idx
        for r, (sib, path) in enumerate(steps):
            log_folded = lmax - 1 - r
            folded = (folded + ro.get(1 << (log_folded + 1), 0)) % P
            evals = [folded, folded]
            evals[(index ^ 1) & 1] = sib
            if len(path) != log_folded or not O.merkle_verify(proof.roots[r], index >> 1, [evals], path, pp):
                return False
            index >>= 1
            folded = O.fold_row(index, log_folded, betas[r], evals[0], evals[1])
        x = pow(O.two_adic_generator(lmax - nr), O.bitrev(index, lmax - nr), P)
        if O.eval_poly(proof.final_poly, x) != folded:
            return False
    return True


# ------------------------------------------------------------ LSPPCS01
def parse(b: bytes) -> Proof:
    """of well-formed bytes (the tests' own proofs): asserts, where the product's parser returns a status"""
    assert b[:8] == b"LSPPCS01"
    nb, nq, nr, nf = struct.unpack_from("<4I", b, 8)
    off = 24

    def u32():
        nonlocal off
        off += 4
        return struct.unpack_from("<I", b, off - 4)[0]

    def fes(n):
        nonlocal off
        off += 32 * n
        out = [int.from_bytes(b[o:o + 32], "little") for o in range(off - 32 * n, off, 32)]
        assert all(v < P for v in out)
        return out

    shape = [[(u32(), u32()) for _ in range(u32())] for _ in range(nb)]
    ys = [[[fes(w) for _ in range(n)] for w, n in bt] for bt in shape]
    roots, final_poly, pow_w = fes(nr), fes(nf), fes(1)[0]
    queries = []
    for _ in range(nq):
        inputs = [([fes(w) for w, _ in bt], fes(u32())) for bt in shape]
        steps = [(fes(1)[0], fes(u32())) for _ in range(nr)]
        queries.append((inputs, steps))
    assert off == len(b)
    return Proof(shape, ys, roots, final_poly, pow_w, queries)


def serialize(p: Proof) -> bytes:
    fe = O.to_canon_bytes
    out = bytearray(b"LSPPCS01")
    out += struct.pack("<4I", len(p.shape), len(p.queries), len(p.roots), len(p.final_poly))
    for b in p.shape:
        out += struct.pack("<I", len(b))
        for w, n in b:
            out += struct.pack("<2I", w, n)
    for v in [v for b in p.ys for m in b for pt in m for v in pt] + list(p.roots) + list(p.final_poly):
        out += fe(v)
    out += fe(p.pow_witness)
    for inputs, steps in p.queries:
        for rows, path in inputs:
            for v in [v for r in rows for v in r]:
                out += fe(v)
            out += struct.pack("<I", len(path))
            for v in path:
                out += fe(v)
        for sib, path in steps:
            out += fe(sib) + struct.pack("<I", len(path))
            for v in path:
                out += fe(v)
    return bytes(out)
