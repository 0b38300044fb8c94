"""The adversarial word corpus (tests/adversarial_words.py) on the CPU:
* its invariants (canonical, no duplicates, 29-form preimages, pairs summing to r);
* the two oracles agree on it -- oracle/lsp_oracle.c (4 x 64-bit limbs, the GPU
  reference at the larger shapes of tests/test_gpu_adversarial_words.py)
  against oracle/pyoracle.py (Python integers);
* the library's host code against Python integers on it: lsp_fr_mul,
  lsp_fr_inv, lsp_fri_fold_row and the host tree tops' lazy 64-bit / IFMA
  Poseidon2 (lsp_host_hash_rows, lsp_host_compress_batch);
* the integer model of the device's 29-bit product (tests/test_f29_bounds.py
  f29_mul) over all ordered corpus pairs: the worst 64-bit column sum.
Everything is integer arithmetic mod r: bit-exact."""
import ctypes
import itertools
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import adversarial_words as A  # noqa: E402
import test_f29_bounds as F29  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

P = O.P


def c_ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


# ------------------------------------------------------------ the corpus
def test_corpus_invariants():
    assert A.R == P == F29.R
    assert all(isinstance(w, int) and 0 <= w < P for w in A.CORPUS)
    assert len(set(A.CORPUS)) == len(A.CORPUS) == A.N >= 48
    assert A.CORPUS[:len(A.BASE)] == A.BASE
    assert len(A.PREIMAGES) == len(A.BASE)
    for w, pre in zip(A.BASE, A.PREIMAGES):
        assert pre in A.CORPUS and pre * 32 % P == w
    # the saturated words are what they claim to be
    assert F29.limbs(A.W_SAT) == [A.M29] * 8 + [(P >> 232) - 1]
    assert F29.limbs((P >> 232) << 232) == [0] * 8 + [P >> 232]
    assert [(A.BASE[11] >> (32 * i)) & A.M32 for i in range(8)] == [A.M32] * 7 + [(P >> 224) - 1]
    s = set(A.CORPUS)
    pairs = sum(1 for w in A.CORPUS if w and P - w in s)
    assert pairs >= len(A.BASE)                       # word sums of exactly r ...
    assert any(P - w - 1 in s for w in A.CORPUS)      # ... r - 1 ...
    assert any(w > 1 and P - w + 1 in s for w in A.CORPUS)  # ... and r + 1
    # array round trip: the limbs are the word, the value is W / 2^256
    a = A.arr(A.CORPUS)
    assert a.shape == (A.N, 4) and A.words_of(a) == A.CORPUS
    assert A.values(a) == [A.value(w) for w in A.CORPUS]


def test_open_phase_points_are_off_the_cosets():
    """z^N = shift^N would put z on the coset shift * H_N, where the open
    stage has no inverse denominators; N = 2^11 covers every smaller power of
    two (z^n = s^n implies z^2n = s^2n)"""
    assert all(w in A.INDEX for w in A.Z_WORDS + A.SHIFT_WORDS)
    for s in A.SHIFT_WORDS:
        assert A.value(s) != 0
        for z in A.Z_WORDS:
            assert pow(A.value(z), 1 << 11, P) != pow(A.value(s), 1 << 11, P)


def test_fillings_shapes():
    h, w, W = 6, 5, A.W_SAT
    f = A.fillings(h, w, W)
    assert tuple(f) == A.FILLINGS
    assert all(len(m) == h and all(len(r) == w for r in m) for m in f.values())
    assert f["const"][3][2] == W and f["by_column"][4][3] == A.CORPUS[3]
    assert f["cyclic"][2][1] == A.CORPUS[15] and f["alternate"][0][0] == W and f["alternate"][1][4] == 0
    assert sum(x != 0 for r in f["spike"] for x in r) == 1
    assert A.mat(f["cyclic"]).shape == (h, w, 4)
    # the index form used at the large shapes is the same matrix
    for hh, ww in ((h, w), (1, 1), (2, 3), (A.N + 3, 9)):
        for name, rows in A.fillings(hh, ww, P - 1).items():
            idx = A.fill_index(name, hh, ww, P - 1)
            assert np.array_equal(A.index_mat(idx), A.mat(rows)), (name, hh, ww)
            assert A.index_values(idx) == [[A.value(x) for x in r] for r in rows]


# ------------------------------------------- C oracle against Python oracle
def test_oracles_agree_on_permutation(oracle_lib):
    pp = O.setup_from_seed().perm
    p = oracle_lib.setup()
    heavy = A.heaviest(10)
    triples = list(itertools.product(heavy, repeat=3))
    st = A.arr([x for t in triples for x in t], (len(triples), 3))
    for i in range(len(triples)):
        oracle_lib.lib().lo_poseidon2_permute(ctypes.byref(p), c_ptr(st[i]))
    exp = [x for t in triples for x in O.permute([A.value(w) for w in t], pp)]
    assert A.values(st) == exp


@pytest.mark.parametrize("w", [1, 2, 3, 7])
def test_oracles_agree_on_hash_iter(oracle_lib, w):
    pp = O.setup_from_seed().perm
    p = oracle_lib.setup()
    rows = A.cyclic(A.N, w)
    m = A.mat(rows)
    out = np.zeros((A.N, 4), np.uint64)
    for i in range(A.N):
        oracle_lib.lib().lo_hash_iter(ctypes.byref(p), c_ptr(m[i]), ctypes.c_size_t(w), c_ptr(out[i]))
    assert A.values(out) == [O.hash_iter([A.value(x) for x in r], pp) for r in rows]


@pytest.mark.parametrize("name", A.FILLINGS)
def test_oracles_agree_on_coset_lde(oracle_lib, name):
    h, w, added = 16, 4, 1
    for W, shift_words in ((A.W_SAT, [A.CORPUS[3]] * w), (P - 1, A.NONZERO[5:5 + w])):
        rows = A.fillings(h, w, W)[name]
        m, sh = A.mat(rows), A.arr(shift_words)
        out = np.zeros((h << added, w, 4), np.uint64)
        oracle_lib.lib().lo_coset_lde_batch(c_ptr(m), ctypes.c_size_t(h), ctypes.c_size_t(w), added, c_ptr(sh),
                                            c_ptr(out), 2)
        vrows = [[A.value(x) for x in r] for r in rows]
        exp = O.coset_lde_batch(vrows, added, [A.value(s) for s in shift_words])
        assert A.values(out) == [x for r in exp for x in r]


def const_perm_trace(log_n, ncols, alpha, delta, start=0):
    """a valid permutation trace whose a and b columns are constant corpus
    words (b = a rotated by one row): (cfgs, rows of values)"""
    n = 1 << log_n
    heavy = A.heaviest(start + ncols)[start:]
    a = [[A.value(wd)] * n for wd in heavy]
    cfg, cols = O.perm_witness(a, [c[1:] + c[:1] for c in a], alpha, delta)
    return [cfg], O.columns_to_rows(cols)


@pytest.mark.parametrize("ncols,start", [(3, 0), (3, 3), (6, 0)])
def test_oracles_agree_on_quotient_values(oracle_lib, ncols, start):
    """h = 4: the C oracle's quotient (lo_prove's debug vectors) on a trace of
    constant saturated columns against pyoracle's quotient_values on the C
    oracle's own LDE, and the two proofs byte for byte"""
    s = O.setup_from_seed()
    p = oracle_lib.setup()
    log_h = 2
    cfgs, rows = const_perm_trace(log_h, ncols, s.alpha, s.delta, start)
    w = len(rows[0])
    buf = oracle_lib.fr_buf([x for r in rows for x in r])
    proof, dbg = oracle_lib.prove(p, buf, 1 << log_h, w, oracle_lib.air_desc(cfgs), debug=True)
    N = (1 << log_h) << 3
    lde = oracle_lib.buf_to_ints(dbg["trace_lde"], N * w)
    lde_rows = [lde[i * w:(i + 1) * w] for i in range(N)]
    assert lde_rows == O.coset_lde_batch(rows, 3, O.GENERATOR)
    alpha = O.from_mont_bytes(bytes(dbg["challenges"])[:32])
    log_q = O.log_quotient_degree(cfgs)
    exp = O.quotient_values(cfgs, lde_rows, log_h, log_q, alpha, [s.alpha, s.delta])
    assert oracle_lib.buf_to_ints(dbg["quotient"], len(exp)) == exp
    assert proof == O.serialize_proof(O.prove(cfgs, rows, [s.alpha, s.delta], s.perm))


# --------------------------------------- the library's host code, on words
def test_host_fr_mul_all_ordered_pairs(product_lib):
    a = A.arr(A.CORPUS)
    out = np.zeros(4, np.uint64)
    rinv = pow(1 << 256, -1, P)
    mul = product_lib.lsp_fr_mul
    ptrs = [a[i].ctypes.data for i in range(A.N)]
    for i, x in enumerate(A.CORPUS):
        for j, y in enumerate(A.CORPUS):
            mul(ptrs[i], ptrs[j], out.ctypes.data)
            assert A.words_of(out)[0] == x * y * rinv % P, (hex(x), hex(y))


def test_host_fr_inv_every_nonzero_word(product_lib):
    a = A.arr(A.NONZERO)
    out = np.zeros(4, np.uint64)
    r2 = pow(1 << 256, 2, P)
    for i, x in enumerate(A.NONZERO):
        product_lib.lsp_fr_inv(a[i].ctypes.data, out.ctypes.data)
        assert A.words_of(out)[0] == pow(x, -1, P) * r2 % P, hex(x)


def test_host_fold_row(product_lib):
    from linea_stark_prover_amd.prover import TwoAdicFriGenericConfig
    heavy = A.heaviest(8)
    for k, (b, e0, e1) in enumerate(itertools.product(heavy, repeat=3)):
        logh = (0, 1, 5, 12)[k % 4]
        idx = (k * 2654435761) % (1 << logh)
        got = TwoAdicFriGenericConfig.fold_row(idx, logh, A.arr([b]), A.arr([e0]), A.arr([e1]))
        assert A.values(got)[0] == O.fold_row(idx, logh, A.value(b), A.value(e0), A.value(e1))
    # e0 + e1 and e0 - e1 on the words that sum to r, r - 1, r + 1
    for k, wd in enumerate(A.CORPUS):
        for e1 in (P - wd, P - wd - 1, P - wd + 1, wd):
            if 0 <= e1 < P:
                got = TwoAdicFriGenericConfig.fold_row(k % 32, 5, A.arr([A.W_SAT]), A.arr([wd]), A.arr([e1]))
                assert A.values(got)[0] == O.fold_row(k % 32, 5, A.value(A.W_SAT), A.value(wd), A.value(e1))


@pytest.fixture(scope="module")
def host_ctx(product_lib):
    from linea_stark_prover_amd.prover import Context, StarkConfig
    ctx = Context(StarkConfig(), device=-1)
    yield ctx
    ctx.close()


def test_host_poseidon2_tree_tops(host_ctx, product_lib):
    """lsp_host_hash_rows / lsp_host_compress_batch: the lazy 64-bit and IFMA
    Poseidon2 of the host tree tops, which carry limb bounds of their own"""
    pp = O.setup_from_seed().perm
    heavy = A.heaviest(12)
    pairs = list(itertools.product(heavy, repeat=2)) + [(A.CORPUS[i], A.CORPUS[(i + 1) % A.N]) for i in range(A.N)]
    pairs += [(w, P - w) for w in A.NONZERO[:60]]
    n = len(pairs)
    m, out = A.arr([x for pr in pairs for x in pr]), np.zeros((n, 4), np.uint64)
    assert product_lib.lsp_host_compress_batch(host_ctx.h, c_ptr(m), n, c_ptr(out)) == 0
    assert A.values(out) == [O.compress(A.value(x), A.value(y), pp) for x, y in pairs]
    for w in (1, 2, 3, 4, 7, 8, 23):
        rows = A.cyclic(A.N, w) + A.const(3, w, A.W_SAT) + A.spike(9, w, P - 1)
        m, out = A.mat(rows), np.zeros((len(rows), 4), np.uint64)
        assert product_lib.lsp_host_hash_rows(host_ctx.h, c_ptr(m), len(rows), w, c_ptr(out)) == 0
        assert A.values(out) == [O.hash_iter([A.value(x) for x in r], pp) for r in rows], f"width {w}"


# ------------------------------------------- the 29-bit product's columns
def test_f29_product_columns_over_corpus_pairs(capsys):
    """the corpus words as 29-bit-limb operands of the device product
    (f29_mul_c, whose asm form drops the 64-bit accumulator's carry-out): the
    worst column sum over all ordered pairs stays below 2^64.  The measured
    maximum is recorded in DESIGN.md beside the model's 2^63.74 for the lazy
    dif4 operand; canonical operands (limbs < 2^29) stay well below it."""
    ops = [F29.limbs(w) for w in A.CORPUS]
    k261 = pow(2, -261, P)
    worst, at = 0, None
    for i, a in enumerate(ops):
        for j, b in enumerate(ops):
            o, wc = F29.f29_mul(a, b)  # asserts every column <= 2^64 - 1
            if wc > worst:
                worst, at = wc, (i, j)
        # the product itself, one partner per word (the model is symmetric in its operands)
        j = (7 * i + 3) % A.N
        o, _ = F29.f29_mul(a, ops[j])
        assert F29.val(o) % P == A.CORPUS[i] * A.CORPUS[j] * k261 % P
    assert worst < 1 << 64
    with capsys.disabled():
        print(f"\n[f29 columns] worst 64-bit column sum over {A.N}^2 corpus pairs: 2^{math.log2(worst):.3f} "
              f"(words {A.CORPUS[at[0]]:#x} x {A.CORPUS[at[1]]:#x})")
