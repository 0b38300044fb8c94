"""The host slice of a Merkle tree (csrc/host_slice.hpp): with
LSP_HOST_SLICE forced to log_frac 1, 2 and 5 the host hashes the last 1/2, 1/4
and 1/32 of the leaves and of every layer below the tree top while the GPU's
launches take the prefix -- and nothing the tree holds may differ from what
LSP_HOST_SLICE=0 makes: every layer and the root of lsp_merkle_commit at 2^6,
2^10, 2^11 and 2^12 rows (the last two straddle the row/quad thresholds with
prefixes that are no powers of two; a lower LSP_HOST_TREE_TOP brings the slice
to the first two), a batch of equal and one of mixed heights, FRI round 0's
tree, whole proofs (also on the debug-bounds library), and openings that end
inside the slice or cross the join.  Everything is bit-exact; each reference is
made once with the slice off.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)
FORCED = (1, 2, 5)
KNOBS = ("LSP_HOST_SLICE", "LSP_HOST_TREE_TOP")


def random_words(rng, h, w):
    """h x w uniformly drawn words below 2^252 (< r): what lies in memory, no conversion"""
    a = rng.integers(0, 1 << 64, size=(h, w, 4), dtype=np.uint64)
    a[..., 3] >>= np.uint64(4)
    return a


class knobs:
    """the two switches, read per call by the library, around a block"""

    def __init__(self, slice_, top=None):
        self.new = {"LSP_HOST_SLICE": str(slice_), "LSP_HOST_TREE_TOP": None if top is None else str(top)}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in KNOBS}
        for k, v in self.new.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def tree_bytes(ctx, arrs, slice_, top=None):
    """-> (root, [layer bytes], tree) of MerkleTreeMmcs.commit under the switches"""
    from linea_stark_prover_amd.prover import MerkleTreeMmcs
    with knobs(slice_, top):
        root, tree = MerkleTreeMmcs(ctx).commit(arrs)
        layers = [tree.layer(k).tobytes() for k in range(tree.height.bit_length())]
    return root.tobytes(), layers, tree


_ref = {}  # (case, top) -> (arrays, root, layers) with the slice off


def reference(ctx, case, top, make):
    if (case, top) not in _ref:
        arrs = make()
        root, layers, _ = tree_bytes(ctx, arrs, 0, top)
        _ref[(case, top)] = (arrs, root, layers)
    return _ref[(case, top)]


def check_tree(ctx, case, top, make, k):
    arrs, root0, layers0 = reference(ctx, case, top, make)
    root, layers, tree = tree_bytes(ctx, arrs, k, top)
    assert root == root0
    assert len(layers) == len(layers0)
    for lvl, (a, b) in enumerate(zip(layers, layers0)):
        assert a == b, f"layer {lvl}"
    return arrs, tree


# default tree top (1024 digests): the trees of 2^6 and 2^10 rows are the
# host's entirely, those of 2^11 and 2^12 rows have GPU levels of 2048 - 2048 >> k
# and 4096 - 4096 >> k leaves ... 1024 - 1024 >> k digests
@pytest.mark.parametrize("k", FORCED)
@pytest.mark.parametrize("w", [1, 3, 8])
@pytest.mark.parametrize("log_h", [6, 10, 11, 12])
def test_layers_and_root(gpu_ctx, log_h, w, k):
    check_tree(gpu_ctx, ("one", log_h, w), None,
               lambda: [random_words(np.random.default_rng(1000 * log_h + w), 1 << log_h, w)], k)


# a tree top of 32 digests: the slice is there from 2^6 rows on (k = 5: one
# digest of the join layer), over the row, quad and -- at 2^12 rows -- every
# narrow level between
@pytest.mark.parametrize("k", FORCED)
@pytest.mark.parametrize("log_h,w", [(6, 3), (10, 1), (10, 8), (12, 3)])
def test_layers_and_root_low_top(gpu_ctx, log_h, w, k):
    check_tree(gpu_ctx, ("one", log_h, w), 32,
               lambda: [random_words(np.random.default_rng(1000 * log_h + w), 1 << log_h, w)], k)


@pytest.mark.parametrize("k", FORCED)
def test_equal_height_batch(gpu_ctx, k):
    """three matrices side by side in every leaf: each one's row range is downloaded"""
    def make():
        rng = np.random.default_rng(77)
        return [random_words(rng, 1 << 12, w) for w in (3, 1, 8)]
    check_tree(gpu_ctx, "batch", None, make, k)


MIXED = [(1 << 12, 2), (1 << 12, 3), (1 << 11, 1), (1 << 7, 5), (1 << 5, 2), (1 << 4, 3), (1 << 1, 1), (1, 7)]


@pytest.mark.parametrize("k", FORCED)
def test_mixed_height_batch(gpu_ctx, k):
    """lsp_merkle_commit_mixed: classes injected inside the slice (2^11, 2^7, and
    2^5 = the layer of the slice's root for k = 5), and above it"""
    from linea_stark_prover_amd.prover import MerkleTreeMmcs

    def make():
        rng = np.random.default_rng(78)
        return [random_words(rng, h, w) for h, w in MIXED]
    arrs, tree = check_tree(gpu_ctx, "mixed", None, make, k)
    mmcs = MerkleTreeMmcs(gpu_ctx)
    root = np.frombuffer(_ref[("mixed", None)][1], np.uint64).reshape(1, 4).copy()
    hs, ws = [h for h, _ in MIXED], [w for _, w in MIXED]
    for i in (0, (1 << 12) - 1, (1 << 12) - (1 << 12 >> k), (1 << 12) - (1 << 12 >> k) - 1):
        rows, path = mmcs.open_batch(i, tree)
        assert mmcs.verify_batch(root, ws, 12, i, rows, path, heights=hs), i


@pytest.mark.parametrize("k", FORCED)
def test_fri_round0_tree(gpu_ctx, k):
    """FRI round 0 commits to the pairs of its input as the rows of a 2-column
    matrix, with no fold fused into the leaves: at 2^11 leaves, that tree"""
    check_tree(gpu_ctx, "fri0", None, lambda: [random_words(np.random.default_rng(79), 1 << 11, 2)], k)


@pytest.mark.parametrize("k", FORCED)
def test_openings_inside_the_slice_and_across_the_join(gpu_ctx, k):
    """lsp_merkle_open / verify_batch: a path that ends inside the slice (the
    last leaf; the slice's first), and paths from the GPU's side whose siblings
    are the slice's digests (the leaf before the slice; the first leaf, whose
    last sibling covers the slice)"""
    from linea_stark_prover_amd.prover import MerkleTreeMmcs
    log_h, w = 12, 3
    n = 1 << log_h
    arrs, tree = check_tree(gpu_ctx, ("one", log_h, w), None,
                            lambda: [random_words(np.random.default_rng(1000 * log_h + w), n, w)], k)
    _, root0, layers0 = _ref[(("one", log_h, w), None)]
    root = np.frombuffer(root0, np.uint64).reshape(1, 4).copy()
    mmcs = MerkleTreeMmcs(gpu_ctx)
    first = n - (n >> k)
    for i in (n - 1, first, first + 1, first - 1, first - (n >> k), 0):
        rows, path = mmcs.open_batch(i, tree)
        assert rows[0].tobytes() == arrs[0][i].tobytes()
        for lvl in range(log_h):  # the path is the reference tree's siblings
            sib = ((i >> lvl) ^ 1) * 32
            assert path[lvl].tobytes() == layers0[lvl][sib:sib + 32], (i, lvl)
        assert mmcs.verify_batch(root, [w], log_h, i, rows, path), i
        bad = path.copy()
        bad[log_h - 1, 0] ^= np.uint64(1)
        assert not mmcs.verify_batch(root, [w], log_h, i, rows, bad), i


# ------------------------------------------------------------- whole proofs
def _proof_inputs(log_n, ncols=3):
    from linea_stark_prover_amd.air import permutation_air
    from linea_stark_prover_amd.prover import StarkConfig, gen_permutation_trace
    a, d, _ = StarkConfig().seeded()
    return gen_permutation_trace(log_n, ncols, a, d), permutation_air(ncols), np.ascontiguousarray(np.concatenate([a, d]))


_proofs = {}


def reference_proof(ctx, log_n):
    if log_n not in _proofs:
        trace, air, pub = _proof_inputs(log_n)
        with knobs(0):
            _proofs[log_n] = (trace, air, pub, ctx.prove(trace, air, pub))
    return _proofs[log_n]


# 2^12 rows: trees of 2^15 leaves (trace, quotient) and FRI round 0's of 2^14;
# 2^9 rows: FRI round 0 has 2^11 leaves, the trace and quotient trees 2^12
@pytest.mark.parametrize("k", FORCED)
@pytest.mark.parametrize("log_n", [9, 12])
def test_whole_proofs_byte_identical(gpu_ctx, log_n, k):
    trace, air, pub, want = reference_proof(gpu_ctx, log_n)
    with knobs(k):
        got = gpu_ctx.prove(trace, air, pub)
    assert got == want
    assert gpu_ctx.verify(got, air, pub)


DBG_CHILD = r'''
import hashlib, os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from linea_stark_prover_amd import _lib as L
from linea_stark_prover_amd.prover import Context, StarkConfig
import test_gpu_host_slice as T
assert b"debug-bounds" in L.lib().lsp_version()
trace, air, pub = T._proof_inputs(12)
with Context(StarkConfig()) as ctx:
    for k in (0,) + T.FORCED:
        with T.knobs(k):
            p = ctx.prove(trace, air, pub)  # a check that fires fails the call (LSP_E_STATE)
        print("proof", k, hashlib.sha256(p).hexdigest())
print("debug-bounds ok")
'''


def test_whole_proofs_on_the_debug_bounds_library(gpu_ctx):
    """the same 2^12 proofs on liblsp_hip_dbg.so: no bounds check fires in a
    launch of a prefix count, and the proofs are the product library's"""
    from linea_stark_prover_amd import build as B
    assert os.path.exists(B.DBG_LIB), "liblsp_hip_dbg.so not built (python -m linea_stark_prover_amd.build --debug-bounds)"
    want = hashlib.sha256(reference_proof(gpu_ctx, 12)[3]).hexdigest()
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([sys.executable, "-c", DBG_CHILD, ROOT], env=dict(env, LSP_LIB=B.DBG_LIB), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0 and "debug-bounds ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    got = {int(x.split()[1]): x.split()[2] for x in r.stdout.splitlines() if x.startswith("proof ")}
    assert got == {k: want for k in (0,) + FORCED}
