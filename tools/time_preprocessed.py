"""What preprocessed columns save: one AIR of w + wp = 8 columns at 2^log_n rows
in two layouts, alternating in one process on device-resident traces,

  (a)  all 8 columns in the main trace, a type-3 program: what the library
       did before preprocessed columns (the baseline)
  (b)  the first wp columns committed once by lsp_preprocess, a type-4
       program over the other 8 - wp

for wp in {2, 4, 6}: host-to-host medians of lsp_prove / lsp_prove_preprocessed
(serialization included), the paired difference, the phase timings of both
(lsp_last_timings) and the one-time lsp_preprocess.

    python tools/time_preprocessed.py [--log-n 19] [--pairs 9] [--out FILE]

The AIR: every main column j runs x' = x^2 + k over the fixed column j mod wp
(degree 2, one quotient chunk); the fixed columns are a seeded key schedule.
The model to compare against: the trace tree's leaf permutations fall from
ceil(8 / 2) to ceil((8 - wp) / 2) per leaf and the trace LDE in proportion to
the columns; two barycentric jobs, one reduce pass over N x wp and 33 openings
are added.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from linea_stark_prover_amd.air import LineaAIR, ProgramBuilder  # noqa: E402
from linea_stark_prover_amd.field import MODULUS, to_mont  # noqa: E402
from linea_stark_prover_amd.prover import Context, StarkConfig  # noqa: E402

W_ALL = 8


def build_air(wp, layout):
    w = W_ALL - wp
    if layout == "a":
        b = ProgramBuilder(W_ALL)
        f = [b.local[i] for i in range(wp)]
        m, mn = [b.local[wp + j] for j in range(w)], [b.next[wp + j] for j in range(w)]
    else:
        b = ProgramBuilder(w, preprocessed_width=wp)
        f = [b.preprocessed[i] for i in range(wp)]
        m, mn = [b.local[j] for j in range(w)], [b.next[j] for j in range(w)]
    for j in range(w):
        b.when_transition().assert_eq(mn[j], m[j] * m[j] + f[j % wp])
    return LineaAIR([b.build()])


def build_rows(wp, h):
    w = W_ALL - wp
    fixed = [[(7 * r * r + 3 + 11 * i) % MODULUS for i in range(wp)] for r in range(h)]
    x = [5 + j for j in range(w)]
    main = []
    for r in range(h):
        main.append(list(x))
        x = [(x[j] * x[j] + fixed[r][j % wp]) % MODULUS for j in range(w)]
    return fixed, main


def matrix(rows):
    return to_mont([v for r in rows for v in r]).reshape(len(rows), len(rows[0]), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=19)
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    h = 1 << args.log_n
    lines = [f"w + wp = {W_ALL} columns, 2^{args.log_n} rows, {args.pairs} alternating pairs, device-resident traces, ms"]
    with Context(StarkConfig()) as ctx:
        a, d, _ = ctx.config.seeded()
        pub = np.concatenate([a, d])
        for wp in (2, 4, 6):
            fixed, main_rows = build_rows(wp, h)
            fm, mm = matrix(fixed), matrix(main_rows)
            joined = np.ascontiguousarray(np.concatenate([fm, mm], axis=1))
            air_a, air_b = build_air(wp, "a"), build_air(wp, "b")
            t0 = time.perf_counter()
            pre = ctx.preprocess(fm)
            t_pre_first = time.perf_counter() - t0
            t0 = time.perf_counter()
            pre = ctx.preprocess(fm)
            t_pre = time.perf_counter() - t0
            da, db = ctx.dev_alloc(joined.nbytes), ctx.dev_alloc(mm.nbytes)
            ctx.h2d(da, joined)
            ctx.h2d(db, mm)

            def run_a():
                ctx.synchronize()
                t = time.perf_counter()
                p = ctx.prove(da, air_a, pub, h=h, w=W_ALL)
                return time.perf_counter() - t, p

            def run_b():
                ctx.synchronize()
                t = time.perf_counter()
                p = ctx.prove(db, air_b, pub, h=h, w=W_ALL - wp, preprocessed=pre)
                return time.perf_counter() - t, p

            for _ in range(2):
                _, pa = run_a()
                _, pb = run_b()
            assert ctx.verify(pa, air_a, pub) and ctx.verify(pb, air_b, pub, preprocessed=pre)
            ta, tb, phases = [], [], {"a": {}, "b": {}}
            for i in range(args.pairs):
                for which in (("a", "b") if i % 2 == 0 else ("b", "a")):
                    t, _ = run_a() if which == "a" else run_b()
                    (ta if which == "a" else tb).append(t)
                    for name, ms in ctx.last_timings():
                        phases[which].setdefault(name, []).append(ms)
            ctx.dev_free(da)
            ctx.dev_free(db)
            ma, mb = statistics.median(ta) * 1e3, statistics.median(tb) * 1e3
            diff = statistics.median([y - x for x, y in zip(ta, tb)]) * 1e3
            lines.append(f"wp = {wp}: (a) {ma:.2f}  (b) {mb:.2f}  paired (b) - (a) {diff:+.2f} ({100 * diff / ma:+.1f} %); "
                         f"lsp_preprocess {t_pre * 1e3:.2f} (first call {t_pre_first * 1e3:.2f}); "
                         f"proof bytes (a) {len(pa)} (b) {len(pb)}")
            for name in phases["a"]:
                pa_, pb_ = statistics.median(phases["a"][name]), statistics.median(phases["b"].get(name, [0.0]))
                lines.append(f"    {name:52s} (a) {pa_:7.3f}  (b) {pb_:7.3f}  {pb_ - pa_:+.3f}")
            del pre
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
