"""Mixed-height MMCS on the GPU: lsp_merkle_commit_mixed,
its trees' layers and openings, against the two references of
tests/mixed_mmcs_ref.py -- (a) big integers over the oracle's sponge for the
small shapes, (b) the host's Poseidon2 on arrays for the 2^17-leaf tree whose
injecting levels cross every lane form.  Also the lane knobs on a tree that
injects (one child process per setting) and the handles' life cycle at the
smallest shapes, for plain, mixed and lsp_preprocess trees.  Everything is
bit-exact.
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


# ------------------------------------------- the lane knobs on a tree that injects
# The knobs are read once per process, so each setting runs in a child.  With
# LSP_COOP_MAX=4 LSP_PAIR_MAX=16 a 64-leaf tree's levels of 32 nodes take one
# lane, 16 and 8 a pair, 4 and below a quad: all three forms of the plain and of
# the injecting kernel; LSP_ROW_MAX=0 keeps the plain levels off the row form.
KNOB_SETTINGS = {
    "default": {},
    "all_forms": {"LSP_COOP_MAX": "4", "LSP_PAIR_MAX": "16", "LSP_ROW_MAX": "0"},
    "one_lane": {"LSP_COOP_MAX": "0", "LSP_PAIR_MAX": "0", "LSP_ROW_MAX": "0"},
    "quads_to_32k": {"LSP_COOP_MAX": "32768", "LSP_COOP_BS": "256", "LSP_ROW_MAX": "0"},
    "rows_beside_injecting_quads": {"LSP_COOP_MAX": "4", "LSP_PAIR_MAX": "16"},
}
KNOB_LEAVES = (0, 37, 63)

KNOB_CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from linea_stark_prover_amd.field import from_mont
from linea_stark_prover_amd.prover import Context, MerkleTreeMmcs, StarkConfig
import test_gpu_mixed_mmcs as T
out = {}
with Context(StarkConfig()) as ctx:
    mmcs = MerkleTreeMmcs(ctx)
    ladder, plain = T.knob_mats()
    for name, (root, tree) in (("ladder", T.commit_mixed(ctx, T.to_arrays(ladder))),
                               ("plain", mmcs.commit(T.to_arrays(plain)))):
        opens = [mmcs.open_batch(i, tree) for i in T.KNOB_LEAVES]
        out[name] = {"root": from_mont(root), "layers": [from_mont(tree.layer(k)) for k in range(7)],
                     "opens": [[[from_mont(r) for r in rows], from_mont(path)] for rows, path in opens]}
        del tree
print(json.dumps(out))
'''


def knob_mats():
    """the ladder 64, 32, ..., 1 (every level injects) and a plain two-matrix tree of 64 rows"""
    rnd = random.Random(55)
    return R.ladder(6, rnd, widths=(1, 2, 3, 7)), R.random_mats([(64, 3), (64, 2)], rnd)


@pytest.fixture(scope="module")
def knob_reference(pp):
    ladder, plain = knob_mats()
    want, oracle = R.commit(ladder, pp), O.merkle_commit(plain, pp)

    def opens(f, tree):
        return [[[list(r) for r in rows], list(path)] for rows, path in (f(tree, i) for i in KNOB_LEAVES)]

    return {"ladder": {"root": [want.root], "layers": want.layers, "opens": opens(R.open, want)},
            "plain": {"root": [oracle.root], "layers": [list(l) for l in oracle.layers],
                      "opens": opens(O.merkle_open, oracle)}}


_abnormal = []  # the setting whose child crashed or hung: no further child is started


@pytest.mark.parametrize("name", list(KNOB_SETTINGS))
def test_lane_knobs_on_injecting_and_plain_trees(knob_reference, name):
    import json
    assert not _abnormal, f"the child of {_abnormal} ended abnormally; not starting another"
    knobs = ("LSP_COOP_MAX", "LSP_PAIR_MAX", "LSP_COOP_BS", "LSP_ROW_MAX")
    env = {k: v for k, v in os.environ.items() if k not in knobs}
    env.update(KNOB_SETTINGS[name])
    try:
        r = subprocess.run([sys.executable, "-c", KNOB_CHILD, ROOT], env=env, capture_output=True, text=True,
                           timeout=120, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _abnormal.append(name)
        raise
    if r.returncode < 0 or r.returncode > 128:
        _abnormal.append(name)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    for tree in ("ladder", "plain"):
        for part in ("root", "layers", "opens"):
            assert got[tree][part] == knob_reference[tree][part], (name, tree, part)


# ------------------------------------------------ handle life cycle, smallest shapes
def _lifecycle_trees(ctx, kind, leaves, pp):
    """-> (root, tree, root of the same commit without a tree or None, reference layers,
    reference open(i) -> (rows, path), heights, widths)"""
    from linea_stark_prover_amd.field import GENERATOR
    from linea_stark_prover_amd.prover import MerkleTreeMmcs
    lib, rnd = _lib.lib(), random.Random(f"{kind}{leaves}")
    if kind == "preprocess":  # leaves = the rows committed to; the tree is over their LDE
        cols = to_arrays(R.random_mats([(leaves, 3)], rnd))[0]
        pre = ctx.preprocess(cols)
        lde = ctx.coset_lde_batch(cols, ctx.config.log_blowup, to_mont([GENERATOR]))
        mats = [[from_mont(row) for row in lde]]
        want = O.merkle_commit(mats, pp)
        return pre.commit, pre.tree, None, want.layers, lambda i: O.merkle_open(want, i), [len(lde)], [3]
    shapes = {"plain": [(leaves, w) for w in (2, 1, 7)],
              "mixed": {1: [(1, 2), (1, 3)], 2: [(2, 1), (1, 3)], 8: [(8, 2), (2, 3), (8, 1), (1, 7)]}[leaves]}[kind]
    mats = R.random_mats(shapes, rnd)
    arrs = to_arrays(mats)
    hs, ws = [h for h, _ in shapes], [w for _, w in shapes]
    ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    lone = np.zeros((1, 4), np.uint64)
    if kind == "plain":
        root, tree = MerkleTreeMmcs(ctx).commit(arrs)
        ctx._chk(lib.lsp_merkle_commit(ctx.h, ptrs, _sizes(ws), len(arrs), leaves, _lib.LSP_MEM_HOST,
                                       lone.ctypes.data, None))
        want = O.merkle_commit(mats, pp)
        return root, tree, lone, want.layers, lambda i: O.merkle_open(want, i), hs, ws
    root, tree = commit_mixed(ctx, arrs)
    ctx._chk(lib.lsp_merkle_commit_mixed(ctx.h, ptrs, _sizes(ws), _sizes(hs), len(arrs), _lib.LSP_MEM_HOST,
                                         lone.ctypes.data, None))
    want = R.commit(mats, pp)
    return root, tree, lone, want.layers, lambda i: R.open(want, i), hs, ws


@pytest.mark.parametrize("kind", ["plain", "mixed", "preprocess"])
def test_handle_life_cycle_at_the_smallest_shapes(product_lib, pp, kind):
    """a context of its own, so that its trees' and its own release are part of the test"""
    from linea_stark_prover_amd.prover import Context, StarkConfig
    lib, ctx = product_lib, Context(StarkConfig())
    for leaves in (2, 8) if kind == "preprocess" else (1, 2, 8):
        root, tree, lone, layers, ref_open, hs, ws = _lifecycle_trees(ctx, kind, leaves, pp)
        H, levels = len(layers[0]), len(layers) - 1
        assert tree.height == H and from_mont(root) == layers[-1]
        if lone is not None:
            assert lone.tobytes() == root.tobytes()
        n, got_h, got_w = ctypes.c_size_t(), _sizes([0] * len(ws)), _sizes([0] * len(ws))
        assert lib.lsp_tree_dims(tree.handle, got_h, got_w, len(ws), ctypes.byref(n)) == _lib.LSP_OK
        assert (n.value, list(got_h), list(got_w)) == (len(ws), hs, ws)
        for i in range(H):
            rows = np.zeros((sum(ws), 4), np.uint64)
            path = np.full((levels + 1, 4), 0xA5A5A5A5A5A5A5A5, np.uint64)  # one digest more than the path
            assert lib.lsp_merkle_open(tree.handle, i, rows.ctypes.data, path.ctypes.data) == _lib.LSP_OK
            want_rows, want_path = ref_open(i)
            assert from_mont(rows) == [x for r in want_rows for x in r], (leaves, i)
            assert from_mont(path[:levels]) == list(want_path) and len(want_path) == levels, (leaves, i)
            assert (path[levels:] == 0xA5A5A5A5A5A5A5A5).all()  # (all of it where one leaf has an empty path)
        for k in range(levels + 1):
            assert from_mont(tree.layer(k)) == list(layers[k]), (leaves, k)
        past = np.zeros((1, 4), np.uint64)
        assert lib.lsp_merkle_layer(tree.handle, levels + 1, past.ctypes.data) == _lib.LSP_E_ARG
        assert lib.lsp_tree_free(tree.handle) == _lib.LSP_OK
        tree.handle = None
    assert lib.lsp_ctx_destroy(ctx.h) == _lib.LSP_OK
    ctx.h = None


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
