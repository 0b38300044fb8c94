"""Witness generation at its edges (csrc/k_witness.hip, csrc/witness.cpp),
bit-exact against pyoracle's restatement of the reference and, where a host
scan would take minutes, against closed forms (tests/witness_cases.py, proved
against pyoracle in tests/test_witness_cases.py).

The scans: inclusive scans over tiles of 2048 elements (256 threads of 8),
one kernel up to 2048 elements, one level of tile aggregates up to 2048
tiles, a second level above that (n > 2^22).  The inputs telescope, so every
row's expected value depends on that row alone and a tile prefix put in the
wrong place shows at that tile, not only where the column ends.

The occurrence table: open addressing over key_hash (words 0 and 2 of the
Montgomery form) with linear probing; with one column per side the key is the
word quadruple the test passes, so the cases choose their slots.

The generator: k_gen_raw_perm against a model of it, every element.
"""
import os
import sys

import numpy as np
import pytest

from oracle import pyoracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import witness_cases as W  # noqa: E402

pytestmark = pytest.mark.gpu

P = O.P
HOST, DEVICE = 0, 1  # LSP_MEM_HOST, LSP_MEM_DEVICE


@pytest.fixture(scope="module")
def wit_ctx(product_lib):
    """a context of its own: the big cases' wit_* buffers go with it when the module ends"""
    from linea_stark_prover_amd.prover import Context, StarkConfig
    ctx = Context(StarkConfig())
    yield ctx
    ctx.close()


def mont(vals):
    from linea_stark_prover_amd.field import to_mont
    return to_mont(list(vals))


def ints(a):
    from linea_stark_prover_amd.field import from_mont
    return from_mont(a.reshape(-1, 4))


def col_major(cols):
    """columns of integers -> (k, n, 4) Montgomery words, the entry points' input layout"""
    return np.stack([mont(c) for c in cols], axis=0)


def row_major(cols):
    """columns of integers -> the (n, k, 4) trace block"""
    return np.stack([mont(c) for c in cols], axis=1)


def challenge_words():
    al, de = W.challenges()
    return mont([al]), mont([de])


def sentinel(n, w):
    """a trace in which no two words are equal and none is a field element's (top bits set)"""
    return (np.arange(n * w * 4, dtype=np.uint64) + np.uint64(0xFACE << 48)).reshape(n, w, 4)


def call_witness(ctx, kind, inputs, counts, n, trace, col0, mem):
    """lsp_witness_permutation (counts = na, nb; inputs = a, b) or
    lsp_witness_lookup (counts = na, nt, nbc; inputs = a, b, a_filter,
    b_filter) into a copy of `trace`, through host or device memory.
    Returns (return code, message, the trace afterwards)."""
    from linea_stark_prover_amd import _lib as L
    al, de = challenge_words()
    trace = trace.copy()
    tw = trace.shape[1]
    inputs = [np.ascontiguousarray(x) for x in inputs]

    def run(ptrs, tptr):
        if kind == "permutation":
            return L.lib().lsp_witness_permutation(ctx.h, ptrs[0], counts[0], ptrs[1], counts[1], n, al.ctypes.data,
                                                   de.ctypes.data, tptr, tw, col0, mem)
        return L.lib().lsp_witness_lookup(ctx.h, ptrs[0], counts[0], ptrs[1], counts[1], counts[2], ptrs[2], ptrs[3],
                                          n, al.ctypes.data, de.ctypes.data, tptr, tw, col0, mem)

    if mem == HOST:
        rc = run([x.ctypes.data for x in inputs], trace.ctypes.data)
    else:
        bufs = []
        try:
            for x in inputs + [trace]:
                bufs.append(ctx.dev_alloc(x.nbytes))
                ctx.h2d(bufs[-1], x)
            rc = run(bufs[:-1], bufs[-1])
            ctx.d2h(trace, bufs[-1])
        finally:
            for p in bufs:
                ctx.dev_free(p)
    msg = L.lib().lsp_last_error(ctx.h) if rc else b""
    return rc, (msg or b"").decode(), trace


def lookup_inputs(case):
    a, b, af, bf = case
    return [col_major(a), col_major([c for t in b for c in t]), mont(af), col_major(bf)], (len(a), len(b), len(b[0]))


def perm_inputs(case):
    a, b = case
    return [col_major(a), col_major(b)], (len(a), len(b))


# ------------------------------------------------------------ scan shapes
def _raw_trace(ctx):
    from linea_stark_prover_amd.trace import RawTrace
    al, de = challenge_words()
    return RawTrace(ctx, [al, de])


def _first_difference(got, exp):
    bad = np.flatnonzero((got != exp).any(axis=(1, 2)))
    return f"{bad.size} of {got.shape[0]} rows differ, the first at row {bad[0]}" if bad.size else ""


@pytest.mark.parametrize("n", W.PERM_SCAN_SIZES)
def test_product_scan_shapes(wit_ctx, n):
    """the check column (a prefix product) at heights that are no power of
    two: partial last threads and tiles, a last tile of one element, one tile
    against two, every row against the reference"""
    from linea_stark_prover_amd.trace import RawPermutationTrace
    a, b = W.rotation_perm_input(n)
    exp = row_major(W.rotation_perm_columns(n))
    rt = _raw_trace(wit_ctx)
    try:
        rt.push_traces([RawPermutationTrace([mont(c) for c in a], [mont(c) for c in b])], [])
        got = rt.get_trace(host=True)
        assert got.shape == exp.shape
        assert np.array_equal(got, exp), _first_difference(got, exp)
    finally:
        rt.close()


@pytest.mark.parametrize("n", W.LOOKUP_SCAN_SIZES)
def test_sum_scan_shapes(wit_ctx, n):
    """the LogUp column (a prefix sum) and the occurrence table's (r - n) / n
    split at heights that are no power of two, every row against the reference"""
    from linea_stark_prover_amd.trace import RawLookupTrace
    a, b, af, bf = W.rotation_lookup_input(n)
    exp = row_major(W.rotation_lookup_columns(n))
    rt = _raw_trace(wit_ctx)
    try:
        rt.push_traces([], [RawLookupTrace([mont(c) for c in a], [[mont(c) for c in t] for t in b], mont(af),
                                           [mont(f) for f in bf])])
        got = rt.get_trace(host=True)
        assert got.shape == exp.shape
        assert np.array_equal(got, exp), _first_difference(got, exp)
    finally:
        rt.close()


def _random_words(n, seed):
    """n canonical Montgomery word quadruples (< 2^250 < r), distinct but for a chance of 2^-200"""
    w = np.random.default_rng(seed).integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    w[:, 3] &= np.uint64((1 << 58) - 1)
    return w


def _upload_rotated(ctx, words, *, back):
    """device buffers (x, y) with x = words and y[i] = words[(i - 1) mod n]; `back` swaps them"""
    n = words.shape[0]
    x, y = ctx.dev_alloc(n * 32), ctx.dev_alloc(n * 32)
    ctx.h2d(x, words)
    ctx.h2d(y, words[-1:])
    if n > 1:
        ctx.h2d(y + 32, words[:-1])
    return (y, x) if back else (x, y)


def _compare_rows(ctx, trace_ptr, width, rows, expected_rows):
    """the trace's rows `rows` (read back one by one) against rows of integers"""
    exp = mont([v for r in expected_rows for v in r]).reshape(len(rows), width, 4)
    got = np.zeros_like(exp)
    for j, r in enumerate(rows):
        ctx.d2h(got[j], trace_ptr + r * width * 32)
    if not np.array_equal(got, exp):
        bad = [rows[j] for j in np.flatnonzero((got != exp).any(axis=(1, 2)))]
        cols = sorted(set(np.nonzero((got != exp).any(axis=2))[1].tolist()))
        pytest.fail(f"{len(bad)} of {len(rows)} compared rows differ (columns {cols}); the first are {bad[:8]}, "
                    f"tiles {[r // W.SC_TILE for r in bad[:8]]}")


def _values_at(words, n, rows):
    """val(i) for the closed forms: the integers of words at rows, the rows before them and n - 1"""
    need = sorted({n - 1} | set(rows) | {(r - 1) % n for r in rows})
    table = dict(zip(need, ints(words[need])))
    return table.__getitem__


@pytest.mark.parametrize("n", W.PERM_BIG_SIZES)
def test_product_scan_two_levels(wit_ctx, n):
    """more than 2048 tiles: the tile aggregates are themselves scanned in
    tiles.  2048^2 + 1 rows end in a tile of one element whose aggregate is
    the one element of the second level's last tile; 2^22 + 2049 rows end in
    a full tile and a tile of one element.  Rows at both ends, around the tile
    boundaries on either side of the second level's boundary, and 2000 random
    rows, against the closed form."""
    from linea_stark_prover_amd import _lib as L
    ctx = wit_ctx
    words = _random_words(n, n)
    bufs = list(_upload_rotated(ctx, words, back=False))
    try:
        bufs.append(ctx.dev_alloc(n * 4 * 32))
        al, de = challenge_words()
        L.check(L.lib().lsp_witness_permutation(ctx.h, bufs[0], 1, bufs[1], 1, n, al.ctypes.data, de.ctypes.data,
                                                bufs[2], 4, 0, DEVICE), ctx.h)
        rows = W.big_rows(n)
        _compare_rows(ctx, bufs[2], 4, rows, W.rotation_perm_rows(_values_at(words, n, rows), n, rows))
    finally:
        for p in bufs:
            ctx.dev_free(p)


def test_sum_scan_two_levels(wit_ctx):
    """2^22 + 1 rows of a lookup whose A is its table rotated by one row: the
    prefix sum over 2049 tiles, and 2^23 records through the occurrence table,
    every key met by two threads"""
    from linea_stark_prover_amd import _lib as L
    ctx = wit_ctx
    n = W.LOOKUP_BIG_SIZE
    words = _random_words(n, n)
    bufs = list(_upload_rotated(ctx, words, back=True))  # a = b rotated
    try:
        ones = np.tile(mont([1]), (n, 1))
        bufs.append(ctx.dev_alloc(n * 32))
        ctx.h2d(bufs[2], ones)  # one table: the same column of ones serves as a_filter and b_filter
        bufs.append(ctx.dev_alloc(n * 8 * 32))
        al, de = challenge_words()
        L.check(L.lib().lsp_witness_lookup(ctx.h, bufs[0], 1, bufs[1], 1, 1, bufs[2], bufs[2], n, al.ctypes.data,
                                           de.ctypes.data, bufs[3], 8, 0, DEVICE), ctx.h)
        rows = W.big_rows(n)
        _compare_rows(ctx, bufs[3], 8, rows, W.rotation_lookup_rows(_values_at(words, n, rows), n, rows))
    finally:
        for p in bufs:
            ctx.dev_free(p)


# ------------------------------------------------------- occurrence table
@pytest.mark.parametrize("name", W.LOOKUP_TABLE_CASES)
def test_occurrence_table(wit_ctx, name):
    """keys that share a slot and wrap past the table's end, long chains under
    contention, a key in two tables, disabled entries beside enabled ones, one
    key on every row, filters whose low words are zero: the whole block
    against the reference (tests/witness_cases.py describes each case)"""
    from linea_stark_prover_amd import _lib as L
    case = W.LOOKUP_CASES[name]()
    exp = row_major(W.lookup_columns(name))
    inputs, counts = lookup_inputs(case)
    n = len(case[0][0])
    rc, msg, got = call_witness(wit_ctx, "lookup", inputs, counts, n, sentinel(n, exp.shape[1]), 0, HOST)
    assert rc == L.LSP_OK, (rc, msg)
    if not np.array_equal(got, exp):
        cols = sorted(set(np.nonzero((got != exp).any(axis=2))[1].tolist()))
        pytest.fail(f"{name}: {_first_difference(got, exp)}, in columns {cols}")


def test_key_held_by_disabled_entries_only(wit_ctx):
    """the enabled A rows' count finds no enabled table entry: the sum does
    not close, as in the reference -- and the context goes on working"""
    from linea_stark_prover_amd import _lib as L
    case = W.LOOKUP_CASES["only_disabled"]()
    inputs, counts = lookup_inputs(case)
    n = len(case[0][0])
    rc, msg, _ = call_witness(wit_ctx, "lookup", inputs, counts, n, sentinel(n, 8), 0, HOST)
    assert rc == L.LSP_E_STATE, (rc, msg)
    assert "should be 0 on the last row" in msg
    test_occurrence_table(wit_ctx, "first_disabled")


# ------------------------------------- uneven column counts and placement
UNEVEN = [("permutation", k) for k in sorted(W.PERM_CASES)] + [("lookup", k) for k in W.LOOKUP_UNEVEN]


def _uneven(kind, name):
    if kind == "permutation":
        inputs, counts = perm_inputs(W.PERM_CASES[name]())
        return inputs, counts, row_major(W.perm_columns(name))
    inputs, counts = lookup_inputs(W.LOOKUP_CASES[name]())
    return inputs, counts, row_major(W.lookup_columns(name))


@pytest.mark.parametrize("mem", [HOST, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("kind,name", UNEVEN, ids=[f"{k}-{n}" for k, n in UNEVEN])
def test_uneven_column_counts_in_a_wider_trace(wit_ctx, kind, name, mem):
    """na != nb (permutation), na != nbc (lookup): the block's columns against
    the reference, written at column 2 of a trace three columns wider than the
    block; every element outside the block keeps what it held.  A block that
    does not fit the trace's width is refused and nothing is written."""
    from linea_stark_prover_amd import _lib as L
    inputs, counts, exp = _uneven(kind, name)
    n, bw = exp.shape[0], exp.shape[1]
    assert bw == (sum(counts) + 2 if kind == "permutation" else counts[0] + counts[1] * (counts[2] + 3) + 3)
    col0, before = 2, sentinel(n, bw + 3)
    rc, msg, got = call_witness(wit_ctx, kind, inputs, counts, n, before, col0, mem)
    assert rc == L.LSP_OK, (rc, msg)
    assert np.array_equal(got[:, col0:col0 + bw], exp), _first_difference(got[:, col0:col0 + bw], exp)
    assert np.array_equal(got[:, :col0], before[:, :col0]) and np.array_equal(got[:, col0 + bw:], before[:, col0 + bw:])
    rc, msg, got = call_witness(wit_ctx, kind, inputs, counts, n, before, 4, mem)  # one column too far right
    assert rc == L.LSP_E_ARG, (rc, msg)
    assert np.array_equal(got, before)


# ------------------------------------------- CBOR raw traces into a wider trace
def _padded(kind, name):
    """(the case's CBOR bytes, the reference's columns of the case resized with
    zero words to PAD_ROWS rows above its longest column)"""
    golden = os.path.join(HERE, "golden")
    if golden not in sys.path:
        sys.path.insert(0, golden)
    import cbor_enc as C
    if kind == "permutation":
        return C.enc(C.permutation_trace(*W.PERM_CASES[name]())), row_major(W.padded_perm_columns(name))
    return C.enc(C.lookup_trace(*W.LOOKUP_CASES[name]())), row_major(W.padded_lookup_columns(name))


@pytest.mark.parametrize("mem", [HOST, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("kind,name", UNEVEN, ids=[f"{k}-{n}" for k, n in UNEVEN])
def test_raw_trace_push_into_a_wider_trace(wit_ctx, kind, name, mem):
    """lsp_raw_trace_push carves a (na != nb), (a, b, a_filter, b_filter with na
    != nbc, one and two tables) out of one column-major block of the parsed
    CBOR trace.  Height = longest column + 3 (12 or 14 rows), so the columns
    are resized with zero words and every carved pointer differs from its
    neighbours by a column count times the height; the block goes to columns
    2 .. 2 + width - 1 of a trace three columns wider, in host and in device
    memory.  Inside the block: the reference's witness of the zero-padded
    columns (tests/test_witness_cases.py: the reference accepts all four padded
    cases, so none runs at height = longest column); outside: untouched."""
    import ctypes
    from linea_stark_prover_amd import _lib as L
    cbor, exp = _padded(kind, name)
    n, bw = exp.shape[0], exp.shape[1]
    col0, before = 2, sentinel(n, bw + 3)
    al, de = challenge_words()
    got = before.copy()
    h = ctypes.c_void_p()
    L.check(L.lib().lsp_raw_trace_parse(cbor, len(cbor), ctypes.byref(h)))
    dev = None
    try:
        mh, w = ctypes.c_size_t(), ctypes.c_size_t()
        L.check(L.lib().lsp_raw_trace_shape(h, None, None, None, None, ctypes.byref(mh), ctypes.byref(w)))
        assert (mh.value, w.value) == (n - W.PAD_ROWS, bw)
        tptr = got.ctypes.data
        if mem == DEVICE:
            dev = tptr = wit_ctx.dev_alloc(got.nbytes)
            wit_ctx.h2d(dev, got)
        rc = L.lib().lsp_raw_trace_push(wit_ctx.h, h, n, al.ctypes.data, de.ctypes.data, tptr, got.shape[1], col0, mem)
        assert rc == L.LSP_OK, (rc, L.lib().lsp_last_error(wit_ctx.h))
        if mem == DEVICE:
            wit_ctx.d2h(got, dev)
    finally:
        L.lib().lsp_raw_trace_free(h)
        if dev is not None:
            wit_ctx.dev_free(dev)
    assert np.array_equal(got[:, col0:col0 + bw], exp), _first_difference(got[:, col0:col0 + bw], exp)
    assert np.array_equal(got[:, :col0], before[:, :col0]) and np.array_equal(got[:, col0 + bw:], before[:, col0 + bw:])


# --------------------------------------------------------------- generator
def _generated(ctx, log_n, ncols, seed):
    al, de = challenge_words()
    out = np.zeros((1 << log_n, 2 * ncols + 2, 4), np.uint64)
    p = ctx.gen_permutation_trace_device(log_n, ncols, al, de, seed)
    try:
        ctx.d2h(out, p)
    finally:
        ctx.dev_free(p)
    return out


@pytest.mark.parametrize("seed", W.GEN_SEEDS, ids=hex)
@pytest.mark.parametrize("log_n,ncols", W.GEN_SHAPES)
def test_device_generator_matches_model(wit_ctx, log_n, ncols, seed):
    """the bench's input: A's values, B's row map and the witness columns,
    every element, against the model of k_gen_raw_perm under the reference's witness"""
    exp = row_major(W.gen_trace_columns(seed, log_n, ncols))
    got = _generated(wit_ctx, log_n, ncols, seed)
    assert np.array_equal(got, exp), _first_difference(got, exp)


def test_device_generator_depends_on_the_seed_alone(wit_ctx):
    """every rank of a sharded proof generates the trace for itself: one seed
    gives the same bytes on another context, another seed gives other bytes"""
    from linea_stark_prover_amd.prover import Context, StarkConfig
    log_n, ncols = 11, 3
    first = _generated(wit_ctx, log_n, ncols, W.GEN_SEEDS[0])
    with Context(StarkConfig()) as other:
        assert _generated(other, log_n, ncols, W.GEN_SEEDS[0]).tobytes() == first.tobytes()
        second = _generated(other, log_n, ncols, W.GEN_SEEDS[1])
    assert second.tobytes() != first.tobytes()
    assert not np.array_equal(second[:, :ncols], first[:, :ncols])  # other values, not only another shuffle
