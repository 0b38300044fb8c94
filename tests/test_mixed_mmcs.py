"""Mixed-height MMCS on the host: the two references
of tests/mixed_mmcs_ref.py against the equal-height oracle and each other, and
lsp_merkle_verify_mixed against the big-integer one.  Everything is bit-exact;
no GPU is touched (a host-only context).
"""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import mixed_mmcs_ref as R  # noqa: E402
from linea_stark_prover_amd import _lib  # noqa: E402
from linea_stark_prover_amd.field import from_mont, to_mont  # noqa: E402
from oracle import pyoracle as O  # noqa: E402


@pytest.fixture(scope="module")
def host_ctx(product_lib):
    from linea_stark_prover_amd.prover import Context, StarkConfig
    return Context(StarkConfig(), device=-1)


@pytest.fixture(scope="module")
def pp():
    return O.setup_from_seed().perm


def _sizes(v):
    return (ctypes.c_size_t * len(v))(*v)


def _verify(lib, ctx, root, widths, heights, index, rows, path):
    """lsp_merkle_verify_mixed on canonical values: rows = one list per matrix"""
    r = to_mont([root])
    flat = to_mont([x for row in rows for x in row])
    p = to_mont(path) if path else np.zeros((1, 4), np.uint64)
    return lib.lsp_merkle_verify_mixed(ctx.h, r.ctypes.data, _sizes(widths), _sizes(heights), len(widths), index,
                                       flat.ctypes.data, p.ctypes.data)


# the batches of the verifier tests: name -> [(height, width)] in the caller's order
def _batches():
    rnd = random.Random(14)
    out = {f"ladder{b}": [(1 << k, rnd.choice((1, 2, 3, 7))) for k in range(b, -1, -1)] for b in range(6)}
    out["gap_H_4"] = [(32, 3), (4, 7)]
    out["two_in_class"] = [(8, 2), (8, 3), (2, 1), (2, 7)]
    out["unsorted"] = [(2, 3), (16, 1), (4, 2), (16, 7)]  # short, tall, mid, tall
    return out


BATCHES = _batches()


@pytest.fixture(scope="module")
def trees(pp):
    """name -> (a)'s tree, computed once"""
    rnd = random.Random(2024)
    return {name: R.commit(R.random_mats(shapes, rnd), pp) for name, shapes in BATCHES.items()}


@pytest.mark.parametrize("log_h", [0, 1, 3])
@pytest.mark.parametrize("nmats", [1, 3])
def test_reference_equals_oracle_on_equal_heights(pp, log_h, nmats):
    rnd = random.Random(100 * log_h + nmats)
    mats = R.random_mats([(1 << log_h, w) for w in (3, 1, 2)[:nmats]], rnd)
    want, got = O.merkle_commit(mats, pp), R.commit(mats, pp)
    assert got.layers == want.layers
    for i in range(1 << log_h):
        assert R.open(got, i) == O.merkle_open(want, i)
        rows, path = R.open(got, i)
        assert R.verify(got.root, got.heights, i, rows, path, pp)
        assert O.merkle_verify(want.root, i, rows, path, pp)


@pytest.mark.parametrize("log_h", [0, 1, 3])
@pytest.mark.parametrize("nmats", [1, 3])
def test_both_verifiers_walk_the_oracles_openings(product_lib, host_ctx, pp, log_h, nmats):
    """lsp_merkle_verify and lsp_merkle_verify_mixed share one path walk: on an
    equal-height batch both accept every opening of the oracle's tree and both
    reject one flipped word anywhere in it, and a wrong index"""
    H, widths = 1 << log_h, [1, 2, 7][:nmats]
    mats = R.random_mats([(H, w) for w in widths], random.Random(1000 * log_h + nmats))
    tree = O.merkle_commit(mats, pp)

    def both(root, index, rows, path):
        r, flat = to_mont([root]), to_mont([x for row in rows for x in row])
        p = to_mont(path) if path else np.zeros((1, 4), np.uint64)
        plain = product_lib.lsp_merkle_verify(host_ctx.h, r.ctypes.data, _sizes(widths), nmats, log_h, index,
                                              flat.ctypes.data, p.ctypes.data)
        assert plain == _verify(product_lib, host_ctx, root, widths, [H] * nmats, index, rows, path)
        return plain

    for i in range(H):
        rows, path = O.merkle_open(tree, i)
        rows, path = [list(r) for r in rows], list(path)
        assert len(path) == log_h
        assert both(tree.root, i, rows, path) == _lib.LSP_OK, i
        assert both(tree.root ^ 1, i, rows, path) == _lib.LSP_E_VERIFY, i
        for k in range(nmats):  # one flipped word in one element of each matrix's row
            bad = [list(r) for r in rows]
            bad[k][(i + k) % widths[k]] ^= 1 << (64 * (i % 4))
            assert both(tree.root, i, bad, path) == _lib.LSP_E_VERIFY, (i, k)
        for k in range(log_h):  # each path digest in turn
            bad = list(path)
            bad[k] ^= 1 << (64 * (k % 4))
            assert both(tree.root, i, rows, bad) == _lib.LSP_E_VERIFY, (i, k)
        for wrong in ({i ^ 1, (i + 1) % H, H - 1 - i} - {i}) if log_h else ():  # one leaf has one index
            assert both(tree.root, wrong, rows, path) == _lib.LSP_E_VERIFY, (i, wrong)


def test_array_reference_equals_integer_reference(product_lib, host_ctx, pp):
    """H = 2^5, a class at every level, one of them of two matrices"""
    rnd = random.Random(5)
    shapes = [(1 << k, rnd.choice((1, 2, 3, 7))) for k in range(5, -1, -1)] + [(8, 2)]
    mats = R.random_mats(shapes, rnd)
    tree = R.commit(mats, pp)
    arrs = [to_mont([x for row in m for x in row]).reshape(len(m), len(m[0]), 4) for m in mats]
    layers = R.array_layers(product_lib, host_ctx, arrs)
    assert [from_mont(l) for l in layers] == tree.layers
    for i in (0, 13, 31):
        rows, path = R.array_open(arrs, layers, i)
        want_rows, want_path = R.open(tree, i)
        assert from_mont(rows) == [x for r in want_rows for x in r] and from_mont(path) == want_path


@pytest.mark.parametrize("name", list(BATCHES))
def test_verify_accepts_every_opening(product_lib, host_ctx, pp, trees, name):
    t = trees[name]
    for i in range(len(t.layers[0])):
        rows, path = R.open(t, i)
        assert R.verify(t.root, t.heights, i, rows, path, pp)
        assert _verify(product_lib, host_ctx, t.root, t.widths, t.heights, i, rows, path) == _lib.LSP_OK, (name, i)


@pytest.mark.parametrize("name", ["ladder5", "gap_H_4", "two_in_class", "unsorted"])
def test_verify_rejects_tampering(product_lib, host_ctx, pp, trees, name):
    t = trees[name]
    H = len(t.layers[0])
    i = H - 3 if H > 4 else H - 1

    def rc(root=t.root, widths=t.widths, heights=t.heights, index=i, rows=None, path=None):
        r0, p0 = R.open(t, i)
        rows, path = r0 if rows is None else rows, p0 if path is None else path
        assert R.verify(root, heights, index, rows, path, pp) is False
        return _verify(product_lib, host_ctx, root, widths, heights, index, rows, path)

    rows, path = R.open(t, i)
    for k in range(len(rows)):  # one flipped element in each matrix's row
        bad = [list(r) for r in rows]
        bad[k][-1] ^= 1
        assert rc(rows=bad) == _lib.LSP_E_VERIFY, k
    for k in range(len(path)):  # one flipped path digest
        bad = list(path)
        bad[k] ^= 1
        assert rc(path=bad) == _lib.LSP_E_VERIFY, k
    assert rc(index=i ^ 1) == _lib.LSP_E_VERIFY  # a wrong index
    assert rc(root=t.root ^ 1) == _lib.LSP_E_VERIFY


def test_verify_rejects_swaps(product_lib, host_ctx, pp, trees):
    # two rows of one class swapped (equal widths, so only their order differs)
    rnd = random.Random(77)
    t = R.commit(R.random_mats([(8, 3), (2, 2), (8, 3), (2, 2)], rnd), pp)
    rows, path = R.open(t, 5)
    for a, b in ((0, 2), (1, 3)):
        bad = list(rows)
        bad[a], bad[b] = bad[b], bad[a]
        assert not R.verify(t.root, t.heights, 5, bad, path, pp)
        assert _verify(product_lib, host_ctx, t.root, t.widths, t.heights, 5, bad, path) == _lib.LSP_E_VERIFY
    # two heights swapped (equal widths, so the rows parse the same)
    t = R.commit(R.random_mats([(8, 2), (4, 2), (2, 2)], rnd), pp)
    rows, path = R.open(t, 6)
    assert _verify(product_lib, host_ctx, t.root, t.widths, t.heights, 6, rows, path) == _lib.LSP_OK
    for hs in ([8, 2, 4], [4, 8, 2]):
        assert not R.verify(t.root, hs, 6, rows, path, pp)
        assert _verify(product_lib, host_ctx, t.root, t.widths, hs, 6, rows, path) == _lib.LSP_E_VERIFY


def test_status_codes(product_lib, host_ctx, pp, trees):
    t = trees["unsorted"]
    rows, path = R.open(t, 3)

    def rc(widths=t.widths, heights=t.heights, index=3, rws=rows):
        return _verify(product_lib, host_ctx, t.root, widths, heights, index, rws, path)

    assert rc() == _lib.LSP_OK
    assert rc(heights=[2, 16, 6, 16]) == _lib.LSP_E_SIZE  # no power of two
    assert rc(heights=[2, 16, 0, 16]) == _lib.LSP_E_SIZE
    assert rc(widths=[3, 1, 0, 7]) == _lib.LSP_E_ARG     # a zero width
    assert rc(index=16) == _lib.LSP_E_ARG                # index >= H
    assert rc(widths=[], heights=[], rws=[[0]]) == _lib.LSP_E_ARG  # no matrix
    nine = [[0]] * 10
    assert rc(widths=[1] * 10, heights=[16] + [4] * 9, rws=nine) == _lib.LSP_E_ARG  # a ninth matrix in a class
    assert rc(widths=[1] * 10, heights=[16, 16] + [4] * 8, rws=nine) == _lib.LSP_E_VERIFY  # eight are served
    # the commit checks its dimensions before it asks for a GPU
    m = np.zeros((16, 1, 4), np.uint64)
    ptrs = (ctypes.c_void_p * 10)(*[m.ctypes.data] * 10)
    root = np.zeros((1, 4), np.uint64)

    def commit_rc(widths, heights):
        return product_lib.lsp_merkle_commit_mixed(host_ctx.h, ptrs, _sizes(widths), _sizes(heights), len(widths),
                                                   _lib.LSP_MEM_HOST, root.ctypes.data, None)

    assert commit_rc([1, 1], [16, 12]) == _lib.LSP_E_SIZE
    assert commit_rc([1, 0], [16, 4]) == _lib.LSP_E_ARG
    assert commit_rc([1, (1 << 20) + 1], [16, 4]) == _lib.LSP_E_ARG   # widths are held as 32 bits
    assert commit_rc([1, 1 << 63], [16, 4]) == _lib.LSP_E_ARG         # ... and no byte count wraps
    assert commit_rc([1 << 20, 1], [1 << 40, 4]) == _lib.LSP_E_SIZE   # 2^60 elements
    assert commit_rc([1, 1], [1 << 41, 4]) == _lib.LSP_E_SIZE
    assert commit_rc([], []) == _lib.LSP_E_ARG
    assert commit_rc([1] * 10, [16] + [4] * 9) == _lib.LSP_E_ARG
    assert commit_rc([1, 1], [16, 4]) == _lib.LSP_E_STATE  # a sound batch: only the GPU is missing
    # lsp_tree_dims without a tree
    n = ctypes.c_size_t()
    assert product_lib.lsp_tree_dims(None, None, None, 0, ctypes.byref(n)) == _lib.LSP_E_ARG


def test_python_verify_batch_takes_heights(host_ctx, pp, trees):
    from linea_stark_prover_amd.prover import MerkleTreeMmcs
    t = trees["unsorted"]
    mmcs = MerkleTreeMmcs(host_ctx)
    rows, path = R.open(t, 9)
    arr_rows = [to_mont(r) for r in rows]
    assert mmcs.verify_batch(to_mont([t.root]), t.widths, 4, 9, arr_rows, to_mont(path), heights=t.heights)
    assert not mmcs.verify_batch(to_mont([t.root]), t.widths, 4, 8, arr_rows, to_mont(path), heights=t.heights)
    # arguments that do not fit each other are the caller's error, not a rejection
    for kw in (dict(heights=t.heights[:-1]), dict(heights=[2 * h for h in t.heights]),
               dict(heights=t.heights, rows=arr_rows[:-1]), dict(heights=t.heights, path=to_mont(path[:-1]))):
        args = dict(rows=arr_rows, path=to_mont(path))
        args.update(kw)
        with pytest.raises(ValueError):
            mmcs.verify_batch(to_mont([t.root]), t.widths, 4, 9, **args)
    with pytest.raises(_lib.LspError) as e:  # the library's own status for what only it checks
        mmcs.verify_batch(to_mont([t.root]), t.widths, 4, 16, arr_rows, to_mont(path), heights=t.heights)
    assert e.value.code == _lib.LSP_E_ARG
