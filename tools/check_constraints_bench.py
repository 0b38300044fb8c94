"""Time of check_constraints (lsp_check_constraints, csrc/k_check.hip) on
device-resident traces, beside lsp_prove on the same trace in the same process
(diagnostic, not the bench contract).

    python tools/check_constraints_bench.py [--out FILE] [--no-prove] [CASE ...]

CASE: LOG_N (the 3 x 3 permutation AIR, w = 8) or wLOG_N (the wide AIR,
w = 184); default 19 22 w20.  One line per case, printed and written to FILE
(default profiles/check_constraints_bench.txt) under the library's source hash:
the check's time (median of LSP_CCB_REPS = 7 after a warm-up; host wall time
around the synchronous call, so the mask's d2h and the launch are in it),
2 h w 32 B / time (every row is read as `local` and as `next`), the algorithmic
h w 32 B / time against the 8 TB/s of HBM, the kernel's field products per
second (counted from the AIR, as k_check.hip's walker multiplies) against the
device multiplier's calibrated rate (lsp_calibrate_fr_mul), and the proof's time
and the check's share of it (--no-prove: the check alone, for a counter pass
under rocprofv3 --pmc)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from linea_stark_prover_amd.air import AirPermutationConfig, permutation_air  # noqa: E402
from linea_stark_prover_amd.build import library_hash, source_hash  # noqa: E402
from linea_stark_prover_amd.prover import Context, StarkConfig, gen_wide_trace  # noqa: E402

HBM_TBS = 8.0

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                              "profiles", "check_constraints_bench.txt"))
ap.add_argument("--no-prove", action="store_true")
ap.add_argument("cases", nargs="*", default=["19", "22", "w20"])
args = ap.parse_args()
reps = int(os.environ.get("LSP_CCB_REPS", "7"))

lines = [f"lib_src_sha16={library_hash() or source_hash()} check_constraints on device-resident traces, "
         f"median of {reps}"]
print(lines[0], flush=True)
ctx = Context(StarkConfig())
a, d, _ = ctx.config.seeded()
pub = np.concatenate([a, d])


peak = ctx.calibrate_fr_mul()


def products_per_row(air):
    """field products of k_check.hip's check_walk on one row pair"""
    n = 0
    for c in air.configs:
        if isinstance(c, AirPermutationConfig):
            n += 2 * len(c.a_columns_ids) + len(c.b_columns_ids) + 4
        else:
            n += len(c.a_columns_ids) + 3 + len(c.b_columns_ids) * (len(c.b_columns_ids[0]) + 5)
    return n


def median(f):
    f()
    ts = []
    for _ in range(reps):
        ctx.synchronize()
        t = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t)
    return sorted(ts)[len(ts) // 2], r


for case in args.cases:
    wide = case.startswith("w")
    lg = int(case[1:] if wide else case)
    if wide:
        tr, air = gen_wide_trace(lg, a, d)
        h, w = tr.shape[0], tr.shape[1]
        dp = ctx.dev_alloc(tr.nbytes)
        ctx.h2d(dp, tr)
        del tr
    else:
        air, h, w = permutation_air(3), 1 << lg, 8
        dp = ctx.gen_permutation_trace_device(lg, 3, a, d)
    t_chk, rep = median(lambda: ctx.check_constraints(dp, air, pub, h=h, w=w))
    assert rep.ok, str(rep)
    t_prv = None
    if not args.no_prove:
        t_prv, proof = median(lambda: ctx.prove(dp, air, pub, h, w))
        assert ctx.verify(proof, air, pub)
    ctx.dev_free(dp)
    nbytes = h * w * 32
    line = (f"check_constraints 2^{lg} x {w} ({'wide' if wide else '3x3'} AIR, {len(rep.counts)} constraints): "
            f"{t_chk * 1e3:.3f} ms, 2hw32B/t = {2 * nbytes / t_chk / 1e12:.3f} TB/s, "
            f"hw32B/t = {nbytes / t_chk / 1e12:.3f} TB/s = {100 * nbytes / t_chk / 1e12 / HBM_TBS:.1f} % of "
            f"{HBM_TBS:.0f} TB/s; {products_per_row(air)} products per row = "
            f"{h * products_per_row(air) / t_chk / 1e9:.1f} G/s of {peak:.0f} G/s calibrated")
    if t_prv is not None:
        line += f"; lsp_prove {t_prv * 1e3:.2f} ms, check = {100 * t_chk / t_prv:.2f} % of the proof"
    print(line, flush=True)
    lines.append(line)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
