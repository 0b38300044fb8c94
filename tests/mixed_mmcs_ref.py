"""Two references for the mixed-height MMCS, shared
by tests/test_mixed_mmcs.py (CPU) and tests/test_gpu_mixed_mmcs.py.  No tests
in this module.

(a) `commit` / `open` / `verify`: p3-merkle-tree's MerkleTree::new, open_batch
    and verify_batch for DIGEST_ELEMS = 1, restated over Python integers with
    oracle.pyoracle's hash_iter and compress.  Matrices are lists of rows of
    canonical values.
(b) `array_layers`: every layer of the same tree from lsp_host_hash_rows and
    lsp_host_compress_batch (the host's IFMA / scalar Poseidon2, which the CPU
    suites hold to both oracles; not the device's 29-bit kernels), on limb
    arrays.  For the shapes (a) is too slow for.
"""
import ctypes
from dataclasses import dataclass
from typing import List

import numpy as np

from oracle import pyoracle as O


def classes(heights):
    """[(height, [matrix indices in the caller's order])], tallest first (p3's
    stable sort by height)"""
    out = []
    for k in sorted(range(len(heights)), key=lambda k: -heights[k]):
        if not out or out[-1][0] != heights[k]:
            out.append((heights[k], []))
        out[-1][1].append(k)
    return out


# ------------------------------------------------------------------ (a)
@dataclass
class Tree:
    mats: List[List[List[int]]]
    layers: List[List[int]]  # after injection; layers[-1] = [root]

    @property
    def root(self):
        return self.layers[-1][0]

    @property
    def heights(self):
        return [len(m) for m in self.mats]

    @property
    def widths(self):
        return [len(m[0]) for m in self.mats]


def _class_hash(mats, idx, i, pp):
    return O.hash_iter([x for k in idx for x in mats[k][i]], pp)


def commit(mats, pp) -> Tree:
    cls = classes([len(m) for m in mats])
    for h, _ in cls:
        O.log2_strict(h)
    by_height = dict(cls)
    H = cls[0][0]
    layers = [[_class_hash(mats, cls[0][1], i, pp) for i in range(H)]]
    while len(layers[-1]) > 1:
        prev = layers[-1]
        n = len(prev) // 2
        cur = [O.compress(prev[2 * i], prev[2 * i + 1], pp) for i in range(n)]
        if n in by_height:
            cur = [O.compress(cur[i], _class_hash(mats, by_height[n], i, pp), pp) for i in range(n)]
        layers.append(cur)
    return Tree(mats, layers)


def open(tree: Tree, index: int):
    """(one row per matrix in the caller's order, the sibling digests)"""
    H = len(tree.layers[0])
    rows = [list(m[index // (H // len(m))]) for m in tree.mats]
    path = [tree.layers[k][(index >> k) ^ 1] for k in range(len(tree.layers) - 1)]
    return rows, path


def verify(root, heights, index, rows, path, pp) -> bool:
    cls = classes(heights)
    by_height = dict(cls)
    H = cls[0][0]
    if not 0 <= index < H or len(path) != O.log2_strict(H):
        return False
    cur = O.hash_iter([x for k in cls[0][1] for x in rows[k]], pp)
    for k, sib in enumerate(path):
        cur = O.compress(sib, cur, pp) if (index >> k) & 1 else O.compress(cur, sib, pp)
        n = H >> (k + 1)
        if n in by_height:
            cur = O.compress(cur, O.hash_iter([x for j in by_height[n] for x in rows[j]], pp), pp)
    return cur == root


def ladder(log_h, rnd, widths=(1, 2, 3, 7)):
    """one matrix at every height 2^log_h ... 1, widths drawn from `widths`;
    rnd: a random.Random"""
    return [[[rnd.randrange(O.P) for _ in range(w)] for _ in range(1 << b)]
            for b in range(log_h, -1, -1) for w in [rnd.choice(widths)]]


def random_mats(shapes, rnd):
    """shapes: [(height, width)] in the caller's order"""
    return [[[rnd.randrange(O.P) for _ in range(w)] for _ in range(h)] for h, w in shapes]


# ------------------------------------------------------------------ (b)
def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def array_layers(lib, host_ctx, mats):
    """mats: (h_j, w_j, 4) uint64 arrays in the caller's order -> the layers
    after injection, each an (n, 4) uint64 array"""
    cls = classes([m.shape[0] for m in mats])
    by_height = dict(cls)

    def class_hash(idx):
        rows = np.ascontiguousarray(np.concatenate([mats[k] for k in idx], axis=1))
        out = np.zeros((rows.shape[0], 4), np.uint64)
        assert lib.lsp_host_hash_rows(host_ctx.h, _p(rows), rows.shape[0], rows.shape[1], _p(out)) == 0
        return out

    def compress_pairs(pairs):  # (n, 2, 4) -> (n, 4)
        pairs = np.ascontiguousarray(pairs)
        out = np.zeros((pairs.shape[0], 4), np.uint64)
        assert lib.lsp_host_compress_batch(host_ctx.h, _p(pairs), pairs.shape[0], _p(out)) == 0
        return out

    layers = [class_hash(cls[0][1])]
    while layers[-1].shape[0] > 1:
        cur = compress_pairs(layers[-1].reshape(-1, 2, 4))
        if cur.shape[0] in by_height:
            cur = compress_pairs(np.stack([cur, class_hash(by_height[cur.shape[0]])], axis=1))
        layers.append(cur)
    return layers


def array_open(mats, layers, index):
    """(the opened rows concatenated in the caller's order, (sum w, 4); the path, (log H, 4))"""
    H = layers[0].shape[0]
    rows = np.concatenate([m[index // (H // m.shape[0])] for m in mats], axis=0)
    path = np.array([layers[k][(index >> k) ^ 1] for k in range(len(layers) - 1)], np.uint64).reshape(-1, 4)
    return np.ascontiguousarray(rows), path
