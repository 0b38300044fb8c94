"""lsp_open_reduce (k_reduce_matrix: one matrix's terms of a reduced opening on
the 29-bit product) against the formula in Python integers:

    ro[i] += sum_p (offys[p] - off[p] rr_i) inv[p][i],   rr_i = sum_c alpha^c M[i][c],
    off[p] = offset alpha^(p w),   offys[p] = off[p] sum_c alpha^c ys[p][c],

and the returned offset is offset alpha^(npoints w).  Integer arithmetic mod r:
bit-exact, the whole output.  Shapes: widths either side of one and two row
chunks of three, one to three points (the sum is reduced every two), row counts
either side of one workgroup and a partial last one of three, the alpha powers'
LDS copy past 48 KiB (asked for by attribute) and past the device's LDS per
workgroup (the powers then come from global memory), and every operand r - 1.
The same cases run on the bounds-checked library in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from linea_stark_prover_amd.field import MODULUS as R  # noqa: E402
from linea_stark_prover_amd.field import from_mont, to_mont  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS, POINTS, ROWS = [1, 2, 3, 4, 7], [1, 2, 3], [1, 255, 256, 257, 600]
QTAB_BYTES, APW_BYTES = 3 * 64 * 16, 36  # the reduction table, one alpha power in the 29-bit form


def case(n, w, npts, seed, value=None):
    """M (n x w), inv (npts x n), ys (npts x w), alpha, offset, ro (n) as integers;
    value: every element of M, inv, ys and ro is that"""
    rng = np.random.default_rng(seed)

    def draw(k):
        return [int.from_bytes(rng.bytes(40), "little") % R if value is None else value for _ in range(k)]
    alpha, offset = (int.from_bytes(rng.bytes(40), "little") % R for _ in range(2))
    assert alpha not in (0, 1) and offset not in (0, 1)
    return dict(n=n, w=w, npts=npts, M=draw(n * w), inv=draw(npts * n), ys=draw(npts * w), alpha=alpha,
                offset=offset, ro=draw(n))


def expected(c):
    n, w, npts = c["n"], c["w"], c["npts"]
    apw = [pow(c["alpha"], k, R) for k in range(w)]
    rr = [sum(a * x for a, x in zip(apw, c["M"][i * w:(i + 1) * w])) % R for i in range(n)]
    ro, off = list(c["ro"]), c["offset"]
    for p in range(npts):
        offys = off * sum(a * y for a, y in zip(apw, c["ys"][p * w:(p + 1) * w])) % R
        for i in range(n):
            ro[i] = (ro[i] + (offys - off * rr[i]) * c["inv"][p * n + i]) % R
        off = off * pow(c["alpha"], w, R) % R
    return ro, off


def run(ctx, c):
    """(ro, offset) after lsp_open_reduce, as integers"""
    n, w, npts = c["n"], c["w"], c["npts"]
    ro = to_mont(c["ro"]).reshape(n, 4).copy()
    assert any(c["ro"])  # a nonzero ro on entry
    off = ctx.open_reduce(to_mont(c["M"]).reshape(n, w, 4), to_mont(c["inv"]).reshape(npts, n, 4),
                          to_mont(c["ys"]).reshape(npts, w, 4), to_mont([c["alpha"]]), to_mont([c["offset"]]), ro)
    return from_mont(ro), from_mont(off.reshape(1, 4))[0]


def lds_per_workgroup():
    from test_gpu_preprocessed import _lds_per_workgroup
    lds = _lds_per_workgroup()
    assert lds in (64 * 1024, 160 * 1024), lds
    return lds


def wide_cases():
    """name -> case at n = 4: the alpha powers' LDS copy over 48 KiB, and one
    column past what the device's LDS per workgroup holds beside the table"""
    w_glb = (lds_per_workgroup() - QTAB_BYTES) // APW_BYTES + 1
    assert QTAB_BYTES + APW_BYTES * 1300 > 48 * 1024 >= QTAB_BYTES + APW_BYTES * 1280
    assert QTAB_BYTES + APW_BYTES * w_glb > lds_per_workgroup() >= QTAB_BYTES + APW_BYTES * (w_glb - 1) > 48 * 1024
    return {"over_48k": case(4, 1300, 2, 71), "global": case(4, w_glb, 2, 72)}


@pytest.mark.parametrize("npts", POINTS)
@pytest.mark.parametrize("w", WIDTHS)
def test_open_reduce_is_the_formula(gpu_ctx, w, npts):
    for n in ROWS:
        c = case(n, w, npts, 1000 * w + 10 * npts + n)
        ro, off = expected(c)
        assert run(gpu_ctx, c) == (ro, off), n
        assert off == c["offset"] * pow(c["alpha"], npts * w, R) % R


@pytest.mark.parametrize("name", ["over_48k", "global"])
def test_alpha_powers_beyond_48_kib_and_beyond_the_lds(gpu_ctx, name):
    c = wide_cases()[name]
    assert run(gpu_ctx, c) == expected(c)


def saturated_case():
    return case(257, 7, 3, 73, value=R - 1)


def test_every_operand_r_minus_1(gpu_ctx):
    c = saturated_case()
    assert set(c["M"]) | set(c["inv"]) | set(c["ys"]) | set(c["ro"]) == {R - 1}
    assert run(gpu_ctx, c) == expected(c)


DBG_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from linea_stark_prover_amd import _lib as L
from linea_stark_prover_amd.prover import Context, StarkConfig
import test_gpu_open_reduce as T
assert b"debug-bounds" in L.lib().lsp_version()
with Context(StarkConfig()) as ctx:  # a check that fires fails the call (LSP_E_STATE)
    for c in T.all_cases():
        assert T.run(ctx, c) == T.expected(c), (c["n"], c["w"], c["npts"])
print("debug-bounds ok")
'''


def all_cases():
    cs = [case(n, w, npts, 1000 * w + 10 * npts + n) for w in WIDTHS for npts in POINTS for n in ROWS]
    return cs + list(wide_cases().values()) + [saturated_case()]


def test_debug_bounds_library():
    """the same cases on liblsp_hip_dbg.so: no bounds check fires, the same results"""
    from linea_stark_prover_amd import build as B
    assert os.path.exists(B.DBG_LIB), "liblsp_hip_dbg.so not built (python -m linea_stark_prover_amd.build --debug-bounds)"
    r = subprocess.run([sys.executable, "-c", DBG_CHILD, ROOT], env=dict(os.environ, LSP_LIB=B.DBG_LIB),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "debug-bounds ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
