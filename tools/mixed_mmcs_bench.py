"""One mixed-height tree against one tree per matrix.

    python tools/mixed_mmcs_bench.py [--log-top 20] [--log-bottom 10] [--width 8] [--reps 7]

Commits the ladder 2^log_top x w, 2^(log_top-1) x w, ..., 2^log_bottom x w
(device-resident matrices) as one lsp_merkle_commit_mixed tree, and the same
matrices as separate lsp_merkle_commit trees with LSP_HOST_TREE_TOP=0, so both
sides run every level on the GPU.  Both sides allocate and fill the trees' own
copies of the matrices inside the timed call.  Prints the median of `reps`
timed runs after one warm-up of each side, and the per-matrix medians of the
separate side.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from linea_stark_prover_amd import _lib as L  # noqa: E402
from linea_stark_prover_amd import build as B  # noqa: E402
from linea_stark_prover_amd.prover import Context, StarkConfig  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-top", type=int, default=20)
    ap.add_argument("--log-bottom", type=int, default=10)
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    os.environ["LSP_HOST_TREE_TOP"] = "0"  # read per commit; lsp_merkle_commit_mixed has no host top
    heights = [1 << b for b in range(a.log_top, a.log_bottom - 1, -1)]
    n = len(heights)
    rng = np.random.default_rng(1)
    lib = L.lib()
    with Context(StarkConfig()) as ctx:
        dev = []
        for h in heights:
            m = rng.integers(0, 1 << 64, size=(h, a.width, 4), dtype=np.uint64)
            m[..., 3] >>= np.uint64(4)  # words below 2^252 < r
            dev.append(ctx.dev_alloc(m.nbytes))
            ctx.h2d(dev[-1], m)
        ptrs = (ctypes.c_void_p * n)(*dev)
        ws = (ctypes.c_size_t * n)(*[a.width] * n)
        hs = (ctypes.c_size_t * n)(*heights)
        root = np.zeros((1, 4), np.uint64)

        def mixed():
            t0 = time.perf_counter()
            ctx._chk(lib.lsp_merkle_commit_mixed(ctx.h, ptrs, ws, hs, n, L.LSP_MEM_DEVICE, root.ctypes.data, None))
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def separate():
            each = []
            for k in range(n):
                one = (ctypes.c_void_p * 1)(dev[k])
                t0 = time.perf_counter()
                ctx._chk(lib.lsp_merkle_commit(ctx.h, one, ws, 1, heights[k], L.LSP_MEM_DEVICE, root.ctypes.data,
                                               None))
                ctx.synchronize()
                each.append((time.perf_counter() - t0) * 1e3)
            return each

        mixed(), separate()
        tm, ts = [], []
        for _ in range(a.reps):
            tm.append(mixed())
            ts.append(separate())
        for p in dev:
            ctx.dev_free(p)
    med = statistics.median
    print(f"library {B.library_hash()}  ladder 2^{a.log_top}..2^{a.log_bottom} x {a.width}, {n} matrices, "
          f"median of {a.reps}")
    print(f"one mixed tree         {med(tm):9.3f} ms   (min {min(tm):.3f}, max {max(tm):.3f})")
    tot = [sum(e) for e in ts]
    print(f"{n} separate trees      {med(tot):9.3f} ms   (min {min(tot):.3f}, max {max(tot):.3f})")
    for k, h in enumerate(heights):
        print(f"  2^{h.bit_length() - 1:<2} alone          {med([e[k] for e in ts]):9.3f} ms")


if __name__ == "__main__":
    main()
