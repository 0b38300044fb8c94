"""Mixed-height MMCS on the GPU: lsp_merkle_commit_mixed,
its trees' layers and openings, against the two references of
tests/mixed_mmcs_ref.py -- (a) big integers over the oracle's sponge for the
small shapes, (b) the host's Poseidon2 on arrays for the 2^17-leaf tree whose
injecting levels cross every lane form.  Everything is bit-exact.
"""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import adversarial_words as A  # noqa: E402
import mixed_mmcs_ref as R  # noqa: E402
from linea_stark_prover_amd import _lib  # noqa: E402
from linea_stark_prover_amd.field import from_mont, to_mont  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def pp():
    return O.setup_from_seed().perm


def _sizes(v):
    return (ctypes.c_size_t * len(v))(*v)


def commit_mixed(ctx, arrs, device=False):
    """lsp_merkle_commit_mixed itself (MerkleTreeMmcs.commit takes the
    equal-height entry point when it can) -> (root, MerkleTree)"""
    from linea_stark_prover_amd.prover import MerkleTree
    hs, ws = [a.shape[0] for a in arrs], [a.shape[1] for a in arrs]
    dev = []
    if device:
        for a in arrs:
            dev.append(ctx.dev_alloc(a.nbytes))
            ctx.h2d(dev[-1], a)
    ptrs = (ctypes.c_void_p * len(arrs))(*(dev if device else [a.ctypes.data for a in arrs]))
    root, t = np.zeros((1, 4), np.uint64), ctypes.c_void_p()
    try:
        ctx._chk(_lib.lib().lsp_merkle_commit_mixed(ctx.h, ptrs, _sizes(ws), _sizes(hs), len(arrs),
                                                    _lib.LSP_MEM_DEVICE if device else _lib.LSP_MEM_HOST,
                                                    root.ctypes.data, ctypes.byref(t)))
    finally:
        for p in dev:
            ctx.dev_free(p)
    return root, MerkleTree(ctx, t, max(hs), ws, hs)


def to_arrays(mats):
    return [to_mont([x for row in m for x in row]).reshape(len(m), len(m[0]), 4) for m in mats]


def check_against_integers(ctx, arrs, want, root, tree):
    """root, every layer and the opening at every index against (a)'s tree"""
    from linea_stark_prover_amd.prover import MerkleTreeMmcs
    assert from_mont(root) == [want.root]
    assert [from_mont(tree.layer(k)) for k in range(len(want.layers))] == want.layers
    n, hs, ws = ctypes.c_size_t(), _sizes([0] * len(arrs)), _sizes([0] * len(arrs))
    ctx._chk(_lib.lib().lsp_tree_dims(tree.handle, hs, ws, len(arrs), ctypes.byref(n)))
    assert (n.value, list(hs), list(ws)) == (len(arrs), want.heights, want.widths)
    mmcs = MerkleTreeMmcs(ctx)
    for i in range(len(want.layers[0])):
        rows, path = mmcs.open_batch(i, tree)
        want_rows, want_path = R.open(want, i)
        assert [from_mont(r) for r in rows] == want_rows and from_mont(path) == want_path, i
        assert mmcs.verify_batch(root, want.widths, len(want_path), i, rows, path, heights=want.heights)


SMALL = {f"ladder{b}": None for b in range(7)}
SMALL.update({
    "gap_H_4": [(64, 3), (4, 7)],
    "gap_H_1": [(32, 2), (1, 85)],
    "classes_of_2_and_3": [(16, 2), (16, 1), (4, 3), (4, 7), (4, 1)],
    "unsorted": [(2, 3), (16, 1), (4, 2), (16, 85), (1, 2)],
})


@pytest.mark.parametrize("name", list(SMALL))
def test_small_shapes_against_integers(gpu_ctx, pp, name):
    rnd = random.Random(name)
    if SMALL[name] is None:
        mats = R.ladder(int(name[6:]), rnd, widths=(1, 2, 3, 7, 85))
    else:
        mats = R.random_mats(SMALL[name], rnd)
    arrs = to_arrays(mats)
    check_against_integers(gpu_ctx, arrs, R.commit(mats, pp), *commit_mixed(gpu_ctx, arrs))


def test_device_pointers_and_python_commit(gpu_ctx, pp):
    from linea_stark_prover_amd.prover import MerkleTreeMmcs
    mats = R.random_mats([(4, 2), (32, 3), (8, 1), (32, 7)], random.Random(3))
    arrs, want = to_arrays(mats), R.commit(mats, pp)
    check_against_integers(gpu_ctx, arrs, want, *commit_mixed(gpu_ctx, arrs, device=True))
    root, tree = MerkleTreeMmcs(gpu_ctx).commit(arrs)
    assert tree.heights == [4, 32, 8, 32] and tree.height == 32
    check_against_integers(gpu_ctx, arrs, want, root, tree)


@pytest.mark.parametrize("log_h", [3, 12])
@pytest.mark.parametrize("nmats", [1, 3])
def test_equal_heights_are_the_existing_path(gpu_ctx, log_h, nmats):
    """byte-equal to lsp_merkle_commit: root, every layer, openings"""
    from linea_stark_prover_amd.prover import MerkleTreeMmcs
    rng = np.random.default_rng(100 * log_h + nmats)
    arrs = [random_words(rng, 1 << log_h, w) for w in (3, 1, 8)[:nmats]]
    mmcs = MerkleTreeMmcs(gpu_ctx)
    root0, tree0 = mmcs.commit(arrs)
    root1, tree1 = commit_mixed(gpu_ctx, arrs)
    assert root0.tobytes() == root1.tobytes()
    for k in range(log_h + 1):
        assert tree0.layer(k).tobytes() == tree1.layer(k).tobytes(), k
    idx = range(1 << log_h) if log_h == 3 else rng.integers(0, 1 << log_h, 64).tolist()
    for i in idx:
        (rows0, path0), (rows1, path1) = mmcs.open_batch(i, tree0), mmcs.open_batch(i, tree1)
        assert path0.tobytes() == path1.tobytes() and len(rows0) == len(rows1)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(rows0, rows1))
        assert mmcs.verify_batch(root0, tree0.widths, log_h, i, rows1, path1)


def random_words(rng, h, w):
    """h x w uniformly drawn words below 2^252 (< r): what lies in memory, no conversion"""
    a = rng.integers(0, 1 << 64, size=(h, w, 4), dtype=np.uint64)
    a[..., 3] >>= np.uint64(4)
    return a


# an injecting level in every lane form: single lane (2^16 nodes), pair (2^15),
# quads (2^14, 2^11, 2^10 and below), on both sides of the 128-node width from
# which an equal-height tree finishes in one workgroup, and into the root
CROSSING = [(1 << 17, 2), (1 << 16, 1), (1 << 15, 3), (1 << 14, 2), (1 << 11, 7), (1 << 10, 1), (1 << 7, 3),
            (1 << 6, 2), (1 << 1, 1), (1 << 0, 5)]


def test_lane_form_crossings_against_host_arrays(gpu_ctx, product_lib):
    from linea_stark_prover_amd.prover import Context, MerkleTreeMmcs, StarkConfig
    rng = np.random.default_rng(17)
    arrs = [random_words(rng, h, w) for h, w in CROSSING]
    hs, ws = [h for h, _ in CROSSING], [w for _, w in CROSSING]
    host_ctx = Context(StarkConfig(), device=-1)
    want = R.array_layers(product_lib, host_ctx, arrs)
    root, tree = commit_mixed(gpu_ctx, arrs)
    assert root.tobytes() == want[-1].tobytes()
    for k, layer in enumerate(want):
        assert tree.layer(k).tobytes() == layer.tobytes(), f"layer {k}"
    mmcs = MerkleTreeMmcs(gpu_ctx)

    def verify(i, rows, path):
        return product_lib.lsp_merkle_verify_mixed(host_ctx.h, root.ctypes.data, _sizes(ws), _sizes(hs), len(ws), i,
                                                   rows.ctypes.data, path.ctypes.data)

    for n, i in enumerate(rng.integers(0, 1 << 17, 64).tolist()):
        rows, path = mmcs.open_batch(i, tree)
        rows = np.ascontiguousarray(np.concatenate(rows))
        want_rows, want_path = R.array_open(arrs, want, i)
        assert rows.tobytes() == want_rows.tobytes() and path.tobytes() == want_path.tobytes(), i
        assert verify(i, rows, path) == _lib.LSP_OK, i
        rows[n % rows.shape[0], 0] ^= np.uint64(1)  # one element of one matrix's row, a different one each time
        assert verify(i, rows, path) == _lib.LSP_E_VERIFY, (i, n)
    host_ctx.close()


def test_adversarial_words(gpu_ctx, pp):
    """an H = 2^6 ladder filled cyclically from the corpus: the injected rows'
    sponge and both compressions see the saturated words"""
    widths = (1, 2, 3, 7, 2, 3, 1)
    rows = [A.cyclic(1 << b, w) for b, w in zip(range(6, -1, -1), widths)]
    arrs = [A.mat(r) for r in rows]
    mats = [[[A.value(x) for x in row] for row in m] for m in rows]
    check_against_integers(gpu_ctx, arrs, R.commit(mats, pp), *commit_mixed(gpu_ctx, arrs))


DBG_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from linea_stark_prover_amd import _lib as L
from linea_stark_prover_amd.prover import Context, MerkleTreeMmcs, StarkConfig
import test_gpu_mixed_mmcs as T
assert b"debug-bounds" in L.lib().lsp_version()
out = {}
with Context(StarkConfig()) as ctx:
    for name, arrs in T.debug_cases().items():
        root, tree = T.commit_mixed(ctx, arrs)  # a check that fires fails the call (LSP_E_STATE)
        for k in range(tree.height.bit_length()):
            out[f"{name}_{k}"] = tree.layer(k)
        MerkleTreeMmcs(ctx).open_batch(tree.height - 1, tree)
        del tree
np.savez(sys.argv[2], **out)
print("debug-bounds ok")
'''


def debug_cases():
    rng = np.random.default_rng(29)
    return {"ladder6": [random_words(rng, 1 << b, w) for b, w in zip(range(6, -1, -1), (3, 1, 7, 2, 85, 1, 2))],
            "gap12": [random_words(rng, h, w) for h, w in ((1 << 12, 2), (1 << 8, 3), (1, 1))]}


def test_debug_bounds_library(gpu_ctx, tmp_path):
    """the same trees on liblsp_hip_dbg.so: no bounds check fires, and the
    layers are the product library's"""
    from linea_stark_prover_amd import build as B
    assert os.path.exists(B.DBG_LIB), "liblsp_hip_dbg.so not built (python -m linea_stark_prover_amd.build --debug-bounds)"
    out = str(tmp_path / "dbg.npz")
    r = subprocess.run([sys.executable, "-c", DBG_CHILD, ROOT, out], env=dict(os.environ, LSP_LIB=B.DBG_LIB),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "debug-bounds ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(out)
    for name, arrs in debug_cases().items():
        _, tree = commit_mixed(gpu_ctx, arrs)
        for k in range(tree.height.bit_length()):
            assert got[f"{name}_{k}"].tobytes() == tree.layer(k).tobytes(), (name, k)
