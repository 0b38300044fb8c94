"""Time of the quotient evaluation (lsp_quotient_values, csrc/k_quotient.hip)
for a built-in AIR descriptor and for the same constraints as LSP_AIR_PROGRAM
configs (air.lower: the interpreter of csrc/k_air_prog.hpp with its register
file in LDS), on device-resident LDEs (diagnostic, not the bench contract).

    python tools/air_program_bench.py [--out FILE] [CASE ...]

CASE: LOG_N (the 3 x 3 permutation AIR, w = 8) or wLOG_N (the wide AIR,
w = 184); default 19 w20.  Per case the two descriptors alternate, LSP_APB_REPS
= 7 times each after a warm-up of both, and the medians are reported: host wall
time around the synchronous call (the launch, the domain tables' upload and the
stream's drain are in it).  The kernels' own device times come from a run under
`rocprofv3 --kernel-trace --stats` (k_quotient<false, false> is the built-in
walker, k_quotient<false, true> the program-capable one).  The values of the two
are compared before anything is timed."""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from linea_stark_prover_amd import _lib as L  # noqa: E402
from linea_stark_prover_amd.air import lower, permutation_air  # noqa: E402
from linea_stark_prover_amd.build import library_hash, source_hash  # noqa: E402
from linea_stark_prover_amd.field import GENERATOR, to_mont  # noqa: E402
from linea_stark_prover_amd.prover import Context, StarkConfig, gen_wide_trace  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                              "profiles", "air_program_bench.txt"))
ap.add_argument("cases", nargs="*", default=["19", "w20"])
args = ap.parse_args()
reps = int(os.environ.get("LSP_APB_REPS", "7"))

lines = [f"lib_src_sha16={library_hash() or source_hash()} lsp_quotient_values on device-resident LDEs, built-in "
         f"descriptor vs its lowered program, alternating, median of {reps} (host wall time)"]
print(lines[0], flush=True)
ctx = Context(StarkConfig())
a, d, _ = ctx.config.seeded()
pub = np.ascontiguousarray(np.concatenate([a, d]))
alpha = to_mont([0x9e3779b97f4a7c15])
shift = to_mont([GENERATOR])
lb = ctx.config.log_blowup
lib = L.lib()

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
    dlde = ctx.dev_alloc((h << lb) * w * 32)
    L.check(lib.lsp_coset_lde_batch(ctx.h, dp, h, w, lb, shift.ctypes.data, dlde, L.LSP_MEM_DEVICE), ctx.h)
    ctx.dev_free(dp)
    low = lower(air)
    descs = {}
    for name, x in (("built-in", air), ("program", low)):
        dd = x.descriptor()
        descs[name] = ((ctypes.c_int32 * len(dd))(*dd), len(dd))
    lq = ctypes.c_uint32()
    L.check(lib.lsp_log_quotient_degree(descs["built-in"][0], descs["built-in"][1], ctx.config.public_degree,
                                        ctypes.byref(lq)))
    Q = h << lq.value
    douts = {name: ctx.dev_alloc(Q * 32) for name in descs}

    def run(name):
        desc, n = descs[name]
        L.check(lib.lsp_quotient_values(ctx.h, dlde, h, w, desc, n, pub.ctypes.data, 2, alpha.ctypes.data,
                                        douts[name], L.LSP_MEM_DEVICE), ctx.h)
        ctx.synchronize()

    for name in descs:
        run(name)
    got = {name: np.zeros((Q, 4), np.uint64) for name in descs}
    for name in descs:
        ctx.d2h(got[name], douts[name])
    assert np.array_equal(got["built-in"], got["program"]), "the lowered program's values differ"
    ts = {name: [] for name in descs}
    for _ in range(reps):
        for name in descs:
            ctx.synchronize()
            t = time.perf_counter()
            run(name)
            ts[name].append(time.perf_counter() - t)
    med = {name: sorted(v)[len(v) // 2] for name, v in ts.items()}
    cfgs = low.configs
    line = (f"quotient 2^{lg} x {w} ({'wide' if wide else '3x3'} AIR, Q = 2^{lg + lq.value} points): built-in "
            f"{med['built-in'] * 1e3:.3f} ms, program {med['program'] * 1e3:.3f} ms "
            f"(x{med['program'] / med['built-in']:.2f}; {sum(len(c.ops) for c in cfgs)} ops, "
            f"{max(c.nslots for c in cfgs)} slots, min {min(ts['built-in']) * 1e3:.3f} / "
            f"{min(ts['program']) * 1e3:.3f} ms)")
    print(line, flush=True)
    lines.append(line)
    for p in [dlde] + list(douts.values()):
        ctx.dev_free(p)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
