"""lsp_pcs_open beside the phases of lsp_prove it restates, and one mixed-height
opening beside one opening per matrix.

    python tools/pcs_bench.py [--log-n 19] [--log-top 20] [--log-bottom 10] [--width 8] [--reps 7]

Part 1, the uni-stark shape: a 2^log_n x 8 trace (3x3 permutation AIR) opened at
zeta and zeta w_h, 4 width-1 chunks at zeta.  The chunks are seeded random
columns on the cosets GEN g_Q^j H_h: the opening does the same work on them as
on quotient chunks, and the reduced openings of any committed columns are low
degree.  Median of `reps` lsp_pcs_open calls (host to host, after a warm-up),
beside the sum of the same proof's phases in lsp_prove from last_timings -- as
the prover runs them, and with LSP_FRI_HOST_TAIL=0 LSP_HOST_TREE_TOP=0, when
its FRI rounds too all run on the device.

Part 2: the ladder 2^log_top x w ... 2^log_bottom x w committed and opened at
one point as one batch, against each matrix committed and opened alone.
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
from linea_stark_prover_amd.air import permutation_air  # noqa: E402
from linea_stark_prover_amd.field import from_mont, to_mont  # noqa: E402
from linea_stark_prover_amd.prover import Context, HashChallenger, StarkConfig, TwoAdicFriPcs  # noqa: E402

PHASES = ("compute opened values with Lagrange interpolation", "compute_inverse_denominators", "reduce rows",
          "FRI prover")
med = statistics.median


def random_device_matrix(ctx, rng, h, w):
    m = rng.integers(0, 1 << 64, size=(h, w, 4), dtype=np.uint64)
    m[..., 3] >>= np.uint64(4)  # words below 2^252 < r
    d = ctx.dev_alloc(m.nbytes)
    ctx.h2d(d, m)
    return d


def timed_open(ctx, rounds, observed, reps):
    """median ms of lsp_pcs_open over `rounds` = [(tree, [points per matrix])],
    each call on a fresh challenger that observed `observed` and sampled once"""
    lib = L.lib()
    trees = (ctypes.c_void_p * len(rounds))(*[t.handle for t, _ in rounds])
    pts = [p for _, ps in rounds for p in ps]
    counts = (ctypes.c_size_t * len(pts))(*[p.shape[0] for p in pts])
    flat = np.ascontiguousarray(np.concatenate(pts))
    out = []
    for k in range(reps + 1):
        ch = HashChallenger(ctx)
        ch.observe(observed)
        ch.sample()
        ctx.synchronize()
        proof = ctypes.c_void_p()
        t0 = time.perf_counter()
        ctx._chk(lib.lsp_pcs_open(ctx.h, trees, len(rounds), counts, flat.ctypes.data, ch.handle, ctypes.byref(proof)))
        out.append((time.perf_counter() - t0) * 1e3)
        lib.lsp_pcs_proof_free(proof)
    return out[1:]  # the first call warms the tables and buffers


def prove_phases(ctx, dtrace, h, w, air, pub, reps):
    rows = []
    for k in range(reps + 1):
        ctx.prove(dtrace, air, pub, h=h, w=w)
        t = dict(ctx.last_timings())
        rows.append([t.get(p, 0.0) for p in PHASES])
    return [med(r[i] for r in rows[1:]) for i in range(len(PHASES))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=19)
    ap.add_argument("--log-top", type=int, default=20)
    ap.add_argument("--log-bottom", type=int, default=10)
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from oracle import pyoracle as O
    rng = np.random.default_rng(1)
    print(f"library {B.library_hash()}  median of {a.reps} after one warm-up")
    with Context(StarkConfig()) as ctx:
        pcs, lib = TwoAdicFriPcs(ctx), L.lib()
        # ---- part 1
        h, ncols, q = 1 << a.log_n, 3, 4
        w = 2 * ncols + 2
        al, de, _ = ctx.config.seeded()
        pub = np.concatenate([al, de])
        dtrace = ctx.dev_alloc(h * w * 32)
        ctx._chk(lib.lsp_gen_permutation_trace_device(ctx.h, 1, a.log_n, ncols, al.ctypes.data, de.ctypes.data, dtrace))
        troot, ttree = pcs.commit([dtrace], dims=[(h, w)])
        gq = O.two_adic_generator(a.log_n + 2)
        dchunks = [random_device_matrix(ctx, rng, h, 1) for _ in range(q)]
        qroot, qtree = pcs.commit(dchunks, to_mont([O.GENERATOR * pow(gq, j, O.P) % O.P for j in range(q)]),
                                  dims=[(h, 1)] * q)
        observed = np.concatenate([troot, qroot])
        ch = HashChallenger(ctx)
        ch.observe(observed)
        zeta = from_mont(ch.sample())[0]
        pts = to_mont([zeta, zeta * O.two_adic_generator(a.log_n) % O.P])
        t_open = timed_open(ctx, [(ttree, [pts]), (qtree, [pts[:1]] * q)], observed, a.reps)
        del ttree, qtree
        for d in dchunks:
            ctx.dev_free(d)
        air = permutation_air(ncols)
        as_run = prove_phases(ctx, dtrace, h, w, air, pub, a.reps)
        os.environ["LSP_FRI_HOST_TAIL"], os.environ["LSP_HOST_TREE_TOP"] = "0", "0"  # both read per call
        on_device = prove_phases(ctx, dtrace, h, w, air, pub, a.reps)
        del os.environ["LSP_FRI_HOST_TAIL"], os.environ["LSP_HOST_TREE_TOP"]
        ctx.dev_free(dtrace)
        print(f"# uni-stark shape, 2^{a.log_n} x {w} at 2 points + {q} chunks at 1")
        print(f"lsp_pcs_open                         {med(t_open):9.3f} ms   (min {min(t_open):.3f}, max {max(t_open):.3f})")
        for label, v in (("lsp_prove's phases, as it runs them", as_run),
                         ("... with every FRI round on the device", on_device)):
            print(f"{label:36s} {sum(v):9.3f} ms = " + " + ".join(f"{x:.3f}" for x in v))
        print("    (" + ", ".join(PHASES) + ")")
        # ---- part 2
        heights = [1 << b for b in range(a.log_top, a.log_bottom - 1, -1)]
        dev = [random_device_matrix(ctx, rng, hh, a.width) for hh in heights]
        root, tree = pcs.commit(dev, dims=[(hh, a.width) for hh in heights])
        z = to_mont([zeta])
        t_mixed = timed_open(ctx, [(tree, [z] * len(heights))], root, a.reps)
        del tree
        each = []
        for d, hh in zip(dev, heights):
            r1, t1 = pcs.commit([d], dims=[(hh, a.width)])
            each.append(timed_open(ctx, [(t1, [z])], r1, a.reps))
            del t1
        for d in dev:
            ctx.dev_free(d)
        tot = [sum(e[k] for e in each) for k in range(a.reps)]
        print(f"# ladder 2^{a.log_top}..2^{a.log_bottom} x {a.width}, {len(heights)} matrices, one point each")
        print(f"one mixed opening                    {med(t_mixed):9.3f} ms   (min {min(t_mixed):.3f}, max {max(t_mixed):.3f})")
        print(f"{len(heights)} separate openings                {med(tot):9.3f} ms   (min {min(tot):.3f}, max {max(tot):.3f})")
        for e, hh in zip(each, heights):
            print(f"  2^{hh.bit_length() - 1:<2} alone                        {med(e):9.3f} ms")


if __name__ == "__main__":
    main()
