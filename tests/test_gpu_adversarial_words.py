"""Limb-extreme operands through the code that runs on the device.

The other parity suites draw uniform values; to_mont turns each into a
pseudo-random 256-bit word.  Here the words themselves are chosen
(tests/adversarial_words.py: saturated 29- and 32-bit limbs, a top limb equal
to the modulus's, word pairs summing to exactly r, r - 1 and r + 1, the words
whose kernel-internal 29-bit form is any of these) and laid into matrices by
deterministic fillings (constant, per column, cyclic, alternating with zero,
one spike).  Every kernel that an entry point lets a caller feed chosen words
is run on them at the smallest shapes that reach each of its code paths.

Checker: Python integers / oracle/pyoracle.py where that takes a second or
two, oracle/lsp_oracle.c above (pinned to pyoracle on the same corpus by
tests/test_adversarial_words.py).  Integer arithmetic mod r: bit-exact, the
complete output (a stated row sample for the two large hash_rows calls)."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import adversarial_words as A  # noqa: E402
import check_constraints_ref as ref  # noqa: E402
from linea_stark_prover_amd.field import to_mont  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

P = O.P
PY_MAX = 1 << 13  # output elements up to which pyoracle is the LDE reference
HEAVY = A.heaviest(12)


def c_ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def word_arr(w):
    return A.arr([w])


def val_arr(values, shape=None):
    a = to_mont(values)
    return a if shape is None else a.reshape(tuple(shape) + (4,))


# the points and shifts of the open-phase tests: fixed corpus words, none on a
# coset of another (tests/test_adversarial_words.py asserts z^N != s^N)
Z_WORDS, SHIFT_WORDS = A.Z_WORDS, A.SHIFT_WORDS


# ------------------------------------------------------- LDE / DFT / iDFT
LOGH = [1, 2, 3, 4, 5, 6, 10, 11]
WIDTHS = [1, 3, 8, 11, A.N]  # A.N >= 48 columns: the wide plan and its partial last chunk
FILL_W = {"const": A.W_SAT, "alternate": P - 1, "spike": (P >> 232) << 232}


def fill(name, h, w):
    return A.fill_index(name, h, w, FILL_W.get(name, A.W_SAT))


def shift_modes(w):
    """name -> w shift words: one shared, per column from the corpus, 1 (the word of value 1)"""
    one = (1 << 256) % P
    return {"shared": [A.W_SAT] * w, "per_column": [A.NONZERO[(5 * c + 1) % len(A.NONZERO)] for c in range(w)],
            "one": [one] * w}


def _columns(idx, extra):
    """group the columns of a corpus index matrix (with a per-column extra key):
    (representative columns, map column -> representative)"""
    reps, cmap, seen = [], [], {}
    for c in range(idx.shape[1]):
        key = (idx[:, c].tobytes(), extra[c])
        if key not in seen:
            seen[key] = len(reps)
            reps.append(c)
        cmap.append(seen[key])
    return reps, np.array(cmap)


def _expected_from_columns(idx, extra, col_fn):
    """the expected limb array of a column-wise transform: col_fn(column values,
    extra) -> output column values, computed once per distinct column"""
    reps, cmap = _columns(idx, extra)
    cols = [col_fn([A.VALUES[j] for j in idx[:, c].tolist()], extra[c]) for c in reps]
    n = len(cols[0])
    rep_arr = val_arr([cols[k][i] for i in range(n) for k in range(len(reps))], (n, len(reps)))
    return rep_arr[:, cmap]


def lde_expected(oracle_lib, idx, mat, added, shift_words):
    h, w = idx.shape
    if (h * w) << added <= PY_MAX:
        return _expected_from_columns(idx, shift_words, lambda col, s: O.coset_lde_column(col, added, A.value(s)))
    exp = np.zeros((h << added, w, 4), np.uint64)
    sh = A.arr(shift_words)
    oracle_lib.lib().lo_coset_lde_batch(c_ptr(mat), ctypes.c_size_t(h), ctypes.c_size_t(w), added, c_ptr(sh),
                                        c_ptr(exp), 16)
    return exp


@pytest.mark.parametrize("name", A.FILLINGS)
@pytest.mark.parametrize("added", [1, 3])
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("logh", LOGH)
def test_coset_lde(gpu_ctx, oracle_lib, logh, w, added, name):
    h = 1 << logh
    idx = fill(name, h, w)
    mat = A.index_mat(idx)
    for mode, sw in shift_modes(w).items():
        shift = A.arr(sw) if mode == "per_column" else word_arr(sw[0])
        got = gpu_ctx.coset_lde_batch(mat, added, shift)
        assert np.array_equal(got, lde_expected(oracle_lib, idx, mat, added, sw)), f"shifts {mode}"


_ones_dft = {}


def ref_coset_dft(col, shift):
    """p(shift w_h^j) at row bitrev(j), p's coefficients `col`; a constant
    column is that constant times the transform of all ones"""
    h = len(col)
    if h > 64 and col[0] != 1 and len(set(col)) == 1:
        if (h, shift) not in _ones_dft:
            _ones_dft.clear()
            _ones_dft[(h, shift)] = ref_coset_dft([1] * h, shift)
        return [col[0] * x % P for x in _ones_dft[(h, shift)]]
    s, tw = 1, []
    for c in col:
        tw.append(c * s % P)
        s = s * shift % P
    return O.reverse_slice_index_bits(O.ntt(tw, O.two_adic_generator(O.log2_strict(h))))


_idft = {}


def ref_coset_idft(col, shift):
    """coefficients of the polynomial with values `col` on shift * H_h; a
    constant column is the constant polynomial"""
    key = tuple(col)
    if key not in _idft:
        if len(_idft) > 500:  # kept across the shifts of one case, not across the file
            _idft.clear()
        _idft[key] = [col[0]] + [0] * (len(col) - 1) if len(col) > 64 and len(set(col)) == 1 else O.idft(col)
    si, s, out = O.inv(shift), 1, []
    for x in _idft[key]:
        out.append(x * s % P)
        s = s * si % P
    return out


@pytest.mark.parametrize("sw", [A.W_SAT, None], ids=["w_sat", "plain"])
@pytest.mark.parametrize("name", A.FILLINGS)
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("logh", LOGH)
def test_coset_dft(gpu_ctx, logh, w, name, sw):
    idx = fill(name, 1 << logh, w)
    got = gpu_ctx.coset_dft_batch(A.index_mat(idx), None if sw is None else word_arr(sw)[0])
    sv = 1 if sw is None else A.value(sw)
    assert np.array_equal(got, _expected_from_columns(idx, [sv] * w, ref_coset_dft))


@pytest.mark.parametrize("name", A.FILLINGS)
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("logh", LOGH)
def test_coset_idft(gpu_ctx, logh, w, name):
    idx = fill(name, 1 << logh, w)
    mat = A.index_mat(idx)
    for sw in (A.W_SAT, None, (P >> 232) << 232):
        got = gpu_ctx.coset_idft_batch(mat, None if sw is None else word_arr(sw)[0])
        sv = 1 if sw is None else A.value(sw)
        assert np.array_equal(got, _expected_from_columns(idx, [sv] * w, ref_coset_idft)), f"shift {sw}"


# ------------------------------------------------- permutation and sponge
def test_poseidon2_permute(gpu_ctx):
    pp = O.setup_from_seed().perm
    states = list(itertools.product(HEAVY, repeat=3)) + [tuple(r) for r in A.cyclic(A.N, 3)]
    got = gpu_ctx.poseidon2_permute(A.arr([x for s in states for x in s], (len(states), 3)))
    exp = [x for s in states for x in O.permute([A.value(w) for w in s], pp)]
    assert np.array_equal(got, val_arr(exp, (len(states), 3)))


def oracle_hash_rows(oracle_lib, rows):
    p = oracle_lib.setup()
    n, w = rows.shape[0], rows.shape[1]
    exp = np.zeros((n, 4), np.uint64)
    for i in range(n):
        oracle_lib.lib().lo_hash_iter(ctypes.byref(p), c_ptr(rows[i]), ctypes.c_size_t(w), c_ptr(exp[i]))
    return exp


@pytest.mark.parametrize("w", [1, 2, 3, 4, 7, 8, 23])
def test_hash_rows_quad_form(gpu_ctx, oracle_lib, w):
    """300 rows: 4 lanes per state"""
    for name in ("const", "cyclic", "spike"):
        rows = A.index_mat(fill(name, 300, w))
        assert np.array_equal(gpu_ctx.hash_rows(rows), oracle_hash_rows(oracle_lib, rows)), name


@pytest.mark.parametrize("n", [16385, 32769])
@pytest.mark.parametrize("w,name", [(3, "cyclic"), (8, "cyclic"), (7, "const"), (2, "spike")])
def test_hash_rows_pair_and_single_lane_forms(gpu_ctx, oracle_lib, n, w, name):
    """one past 16384 rows: 2 lanes per state; one past 32768: 1 lane; both
    with a partial last workgroup.  A strided sample of 512 rows and the last
    130 against the C oracle"""
    rows = A.index_mat(fill(name, n, w))
    got = gpu_ctx.hash_rows(rows)
    sample = sorted(set(range(0, n, n // 512)[:512]) | set(range(n - 130, n)))
    assert np.array_equal(got[sample], oracle_hash_rows(oracle_lib, np.ascontiguousarray(rows[sample])))


@pytest.mark.parametrize("logh,host_top", [(3, True), (11, False)])
def test_merkle_commit(gpu_ctx, oracle_lib, monkeypatch, logh, host_top):
    """2^3: hashed on the host; 2^11 with every level on the GPU"""
    from linea_stark_prover_amd.prover import MerkleTreeMmcs
    if not host_top:
        monkeypatch.setenv("LSP_HOST_TREE_TOP", "0")
    h = 1 << logh
    p = oracle_lib.setup()
    for name in A.FILLINGS:
        for widths in ([3], [1, 2]):
            cat = A.index_mat(fill(name, h, sum(widths)))
            mats, o = [], 0
            for w in widths:
                mats.append(np.ascontiguousarray(cat[:, o:o + w]))
                o += w
            root, tree = MerkleTreeMmcs(gpu_ctx).commit(mats)
            layers = np.zeros((2 * h - 1, 4), np.uint64)
            oracle_lib.lib().lo_merkle_commit(ctypes.byref(p), c_ptr(cat), ctypes.c_size_t(h),
                                              ctypes.c_size_t(cat.shape[1]), c_ptr(layers), 8)
            assert np.array_equal(root.reshape(4), layers[-1]), name
            off = 0
            for lv in range(logh + 1):
                assert np.array_equal(tree.layer(lv), layers[off:off + (h >> lv)]), f"{name}, layer {lv}"
                off += h >> lv


# ------------------------------------------------------------ open phase
_scale = {}


def interp_expected(idx, shift, z):
    """p3-interpolation's interpolate_coset (pyoracle's formula) in Python
    integers, the row factors computed once per (h, shift, z)"""
    h, w = idx.shape
    if (h, shift, z) not in _scale:
        g = O.two_adic_generator(O.log2_strict(h))
        coset = O.reverse_slice_index_bits([shift * pow(g, i, P) % P for i in range(h)])  # rows are bit-reversed
        sN = pow(shift, h, P)
        f = (pow(z, h, P) - sN) * O.inv(sN * h % P) % P
        _scale[(h, shift, z)] = ([c * O.inv(z - c) % P for c in coset], f)
    scale, f = _scale[(h, shift, z)]
    rows = idx.tolist()
    return [sum(A.VALUES[rows[i][c]] * scale[i] for i in range(h)) % P * f % P for c in range(w)]


# W x R thread layouts of k_interp_partial: w = 1 -> R = 256, 3 -> 85, 85 -> 3, 86 -> 2, 256 -> 1, 257: a second
# column chunk; 1024 rows per block: a partial block, a full one, two
@pytest.mark.parametrize("w", [1, 3, 85, 86, 256, 257])
@pytest.mark.parametrize("h", [1, 2, 16, 1024, 2048])
def test_interpolate_coset(gpu_ctx, h, w):
    k = (h + w) % 3
    zw, sw = Z_WORDS[k], SHIFT_WORDS[(k + 1) % 3]
    z, s = A.value(zw), A.value(sw)
    assert pow(z, h, P) != pow(s, h, P)
    for name in A.FILLINGS:
        idx = fill(name, h, w)
        got = gpu_ctx.interpolate_coset(A.index_mat(idx), h, word_arr(sw), word_arr(zw))
        assert np.array_equal(got, val_arr(interp_expected(idx, s, z))), name
    if h <= 16:  # the formula above against pyoracle's own
        idx = fill("cyclic", h, w)
        assert interp_expected(idx, s, z) == O.interpolate_coset(A.index_values(idx), s, z)
    _scale.clear()


@pytest.mark.parametrize("log_n", [0, 3, 9])
def test_inverse_denominators(gpu_ctx, log_n):
    """2^9: two workgroups"""
    for sw in SHIFT_WORDS:
        got = gpu_ctx.inverse_denominators(A.arr(Z_WORDS), log_n, word_arr(sw))
        exp = O.inverse_denominators(log_n, A.value(sw), [A.value(z) for z in Z_WORDS])
        assert np.array_equal(got, val_arr([x for r in exp for x in r], (len(Z_WORDS), 1 << log_n)))


@pytest.mark.parametrize("w", [1, 5])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 600])
def test_open_reduce(gpu_ctx, n, w):
    """two matrices reduced one after the other into a running ro, every
    operand from the corpus"""
    npts = 2
    for name, aw in (("cyclic", A.W_SAT), ("const", P - 1), ("alternate", A.PREIMAGES[A.BASE.index(A.W_SAT)])):
        i1, i2 = fill(name, n, w), fill("cyclic", n, 2)
        iinv = (fill("cyclic", npts, n) + 11) % A.N
        iy1, iy2 = (fill("cyclic", npts, w) + 40) % A.N, (fill("by_column", 1, 2) + 3) % A.N
        iro = (fill("cyclic", n, 1) + 5) % A.N
        ro = A.index_mat(iro).reshape(n, 4).copy()
        ro_exp = [r[0] for r in A.index_values(iro)]
        a = A.value(aw)
        off = gpu_ctx.open_reduce(A.index_mat(i1), A.index_mat(iinv), A.index_mat(iy1), word_arr(aw),
                                  val_arr([1]), ro)
        off = gpu_ctx.open_reduce(A.index_mat(i2), A.index_mat(iinv[:1]), A.index_mat(iy2), word_arr(aw), off, ro)
        e = O.open_reduce(A.index_values(i1), A.index_values(iinv), A.index_values(iy1), a, 1, ro_exp)
        e = O.open_reduce(A.index_values(i2), A.index_values(iinv[:1]), A.index_values(iy2), a, e, ro_exp)
        assert np.array_equal(ro, val_arr(ro_exp)), name
        assert np.array_equal(off.reshape(1, 4), val_arr([e])) and e == pow(a, npts * w + 2, P)


@pytest.mark.parametrize("logn", [1, 3, 9, 10])
def test_fri_fold(gpu_ctx, logn):
    from linea_stark_prover_amd.prover import TwoAdicFriGenericConfig
    g = TwoAdicFriGenericConfig(gpu_ctx)
    n = 1 << logn
    for name, bw in (("cyclic", A.W_SAT), ("const", P - 1), ("alternate", (P >> 232) << 232), ("by_column", 2),
                     ("spike", A.PREIMAGES[A.BASE.index(A.W_SAT)])):
        # by_column over 2 columns of n/2 rows: (e0, e1) = (CORPUS[0], CORPUS[1]) in every pair
        idx = fill(name, n // 2, 2).reshape(n, 1) if name == "by_column" else fill(name, n, 1)
        v = A.index_mat(idx).reshape(n, 4)
        vi = [r[0] for r in A.index_values(idx)]
        got = g.fold_matrix(word_arr(bw), v)
        assert np.array_equal(got, val_arr(O.fold_vector(vi, A.value(bw)))), name
        for i in sorted({0, n // 2 - 1, n // 5}):
            e = g.fold_row(i, logn - 1, word_arr(bw), v[2 * i], v[2 * i + 1])
            assert np.array_equal(e.reshape(4), got[i])


# ---------------------------------------------------------- batch inverse
@pytest.mark.parametrize("reps", [18, 52])
def test_batch_inverse(gpu_ctx, reps):
    """the nonzero corpus repeated past 4096 (one workgroup's base case) and
    past 3 * 4096 elements"""
    k = len(A.NONZERO)
    n = k * reps
    assert n > (4096 if reps == 18 else 3 * 4096)
    x = np.tile(A.arr(A.NONZERO), (reps, 1))
    inv = val_arr([pow(A.value(w), -1, P) for w in A.NONZERO])
    assert np.array_equal(gpu_ctx.batch_inverse(x), np.tile(inv, (reps, 1)))


# ----------------------------------------------------- quotient and check
def lookup_air():
    from linea_stark_prover_amd.air import AirLookupConfig, LineaAIR
    return LineaAIR([AirLookupConfig([0, 1], [[2, 3], [4, 5]], 6, [7, 8], 9, [10, 11], [12, 13], 14)])


def _air(which):
    from linea_stark_prover_amd.air import permutation_air
    return permutation_air(3) if which == "perm" else lookup_air()


@pytest.mark.parametrize("which", ["perm", "lookup"])
@pytest.mark.parametrize("h", [4, 64])
def test_quotient_values(gpu_ctx, h, which):
    air = _air(which)
    cfgs = ref.oracle_cfgs(air)
    w = 8 if which == "perm" else 15
    log_h, log_q = O.log2_strict(h), O.log_quotient_degree(cfgs)
    for k, name in enumerate(A.FILLINGS):
        idx = fill(name, h << 3, w)
        aw, pub_w = HEAVY[k], [HEAVY[k + 1], A.PREIMAGES[k + 7]]
        got = gpu_ctx.quotient_values(A.index_mat(idx), h, air, A.arr(pub_w), word_arr(aw))
        exp = O.quotient_values(cfgs, A.index_values(idx), log_h, log_q, A.value(aw), [A.value(x) for x in pub_w])
        assert np.array_equal(got, val_arr(exp)), name


def const_perm_trace(log_n, ncols, alpha, delta):
    """a valid permutation trace whose a and b columns are constant corpus
    words (b = a rotated by one row): (cfgs, rows of values)"""
    n = 1 << log_n
    a = [[A.value(wd)] * n for wd in A.heaviest(ncols)]
    cfg, cols = O.perm_witness(a, [c[1:] + c[:1] for c in a], alpha, delta)
    return [cfg], O.columns_to_rows(cols)


@pytest.mark.parametrize("h", [8, 512])
def test_check_constraints(gpu_ctx, h):
    """the whole report and the violating rows' values; adversarial traces
    break (nearly) every constraint on every row, the constant-column trace none"""
    air = _air("perm")
    pub_w = [A.W_SAT, A.PREIMAGES[A.BASE.index(P - 1)]]
    alpha, delta = A.value(pub_w[0]), A.value(pub_w[1])
    for name in A.FILLINGS:
        idx = fill(name, h, 8)
        exp = ref.oracle_report(air, A.index_values(idx), alpha, delta, 4 * h)
        rep = gpu_ctx.check_constraints(A.index_mat(idx), air, A.arr(pub_w), max_violations=4 * h)
        assert ref.as_dict(rep) == exp and not exp["ok"], name
    cfgs, rows = const_perm_trace(O.log2_strict(h), 3, alpha, delta)
    trace = val_arr([x for r in rows for x in r], (h, 8))
    exp = ref.oracle_report(air, rows, alpha, delta, 16)
    assert exp["ok"] and ref.as_dict(gpu_ctx.check_constraints(trace, air, A.arr(pub_w))) == exp
    t, rr = ref.tamper(trace, rows, h - 1, 7)
    assert ref.as_dict(gpu_ctx.check_constraints(t, air, A.arr(pub_w))) == ref.oracle_report(air, rr, alpha, delta, 16)


# ----------------------------------------------------------------- witness
@pytest.mark.parametrize("n", [8, 1 << 10])
def test_permutation_witness(gpu_ctx, n):
    """a = corpus columns, b = a rotated by three rows; alpha and delta corpus
    words for which no row combination + delta is zero"""
    from linea_stark_prover_amd.trace import RawPermutationTrace, RawTrace
    w = 3
    ia = fill("cyclic", n, w)
    ib = np.roll(ia, 3, axis=0)
    aw, dw = A.W_SAT, A.PREIMAGES[A.BASE.index((P >> 232) << 232)]
    al, de = A.value(aw), A.value(dw)
    a = [list(c) for c in zip(*A.index_values(ia))]
    b = [list(c) for c in zip(*A.index_values(ib))]
    for i in range(n):
        assert (O._horner([col[i] for col in a], range(w), al) + de) % P != 0
    cfg, cols = O.perm_witness(a, b, al, de)
    rt = RawTrace(gpu_ctx, [word_arr(aw), word_arr(dw)])
    try:
        am, bm = A.index_mat(ia), A.index_mat(ib)
        rt.push_traces([RawPermutationTrace([np.ascontiguousarray(am[:, c]) for c in range(w)],
                                            [np.ascontiguousarray(bm[:, c]) for c in range(w)])], [])
        got = rt.get_trace(host=True)
    finally:
        rt.close()
    assert np.array_equal(got, np.stack([to_mont(c) for c in cols], axis=1))
    assert np.array_equal(got[:, :w], am) and np.array_equal(got[:, w:2 * w], bm)


# -------------------------------------------------------- one whole proof
@pytest.mark.parametrize("ncols", [3, 6])
def test_whole_proof_of_constant_saturated_columns(gpu_ctx, oracle_lib, ncols):
    """the only way chosen words reach k_reduce_rows, the quotient input and
    the trace LDE inside lsp_prove: constant a and b columns of the heaviest
    words.  Byte-identical to the oracle's proof, and it verifies"""
    from linea_stark_prover_amd.air import permutation_air
    log_n = 5
    p = oracle_lib.setup()
    pub = np.concatenate([np.array(p.alpha, np.uint64).reshape(1, 4), np.array(p.delta, np.uint64).reshape(1, 4)])
    alpha, delta = A.values(pub)
    cfgs, rows = const_perm_trace(log_n, ncols, alpha, delta)
    w = len(rows[0])
    trace = val_arr([x for r in rows for x in r], (1 << log_n, w))
    assert A.words_of(trace[7, :ncols]) == A.heaviest(ncols) == A.words_of(trace[8, ncols:2 * ncols])
    air = permutation_air(ncols)
    assert air.descriptor() == oracle_lib.air_desc(cfgs)
    got = gpu_ctx.prove(trace, air, pub)
    assert got == oracle_lib.prove(p, trace.ctypes.data, 1 << log_n, w, oracle_lib.perm_air(ncols))
    assert gpu_ctx.verify(got, air, pub)
    assert oracle_lib.verify(p, got, oracle_lib.perm_air(ncols)) == 0
