"""The stage API and the prover share one driver per stage (csrc/stages.cpp),
and with it the context's power tables, the cached selector inverses and the
stage buffers.  A stage call between two proofs therefore touches state the
next proof reads: proofs and stage results must not depend on what ran before.

Own short-lived contexts (the session context's caches play no part), the
default StarkConfig, a 3x3 permutation AIR at 2^5 rows.  Integer arithmetic
mod r: every comparison is bit-exact.
"""
import numpy as np
import pytest

from oracle import pyoracle as O
from test_gpu_parity import _perm_setup, _pub, rand_fr

pytestmark = pytest.mark.gpu

LOGN, NCOLS = 5, 3


def _stage_calls(ctx, log):
    """interpolate_coset, inverse_denominators and fri_fold at 2^log, on inputs fixed by `log`"""
    from linea_stark_prover_amd.field import to_mont
    from linea_stark_prover_amd.prover import TwoAdicFriGenericConfig
    rng = np.random.default_rng(7000 + log)
    n = 1 << log
    gen = to_mont([O.GENERATOR])
    mat, z, pts = rand_fr(rng, (n, 3)), rand_fr(rng, (1,)), rand_fr(rng, (2,))
    v, beta = rand_fr(rng, (n,)), rand_fr(rng, (1,))
    return [ctx.interpolate_coset(mat, n, gen, z), ctx.inverse_denominators(pts, log, gen),
            TwoAdicFriGenericConfig(ctx).fold_matrix(beta, v)]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_stage_calls_between_proofs_change_nothing(product_lib, oracle_lib):
    from linea_stark_prover_amd.air import permutation_air
    from linea_stark_prover_amd.prover import Context, StarkConfig
    s, p, trace, w = _perm_setup(LOGN, NCOLS, oracle_lib)
    air, pub = permutation_air(NCOLS), _pub(p)
    h = 1 << LOGN
    _, dbg = oracle_lib.prove(p, trace.ctypes.data, h, w, oracle_lib.perm_air(NCOLS), debug=True)
    lde = np.frombuffer(dbg["trace_lde"].raw, dtype=np.uint64).reshape(h << 3, w, 4).copy()
    alpha = np.array(dbg["challenges"][0:4], dtype=np.uint64).reshape(1, 4)
    quotient = np.frombuffer(dbg["quotient"].raw, dtype=np.uint64).reshape(-1, 4)

    with Context(StarkConfig()) as a:  # proves, and makes no stage call
        proof = a.prove(trace, air, pub)

    with Context(StarkConfig()) as b:
        # the proof's own (log_h, logQ): this call fills the selector cache the proof will read
        first_q = b.quotient_values(lde, h, air, pub, alpha)
        first = {log: _stage_calls(b, log) for log in (4, 6)}
        assert np.array_equal(first_q, quotient)
        got = b.prove(trace, air, pub)
        assert got == proof
        assert b.verify(got, air, pub)
        assert np.array_equal(b.quotient_values(lde, h, air, pub, alpha), first_q)
        for log in (4, 6):
            assert _same(_stage_calls(b, log), first[log])
        # once more the other way round: stage calls, then a proof
        assert _same(_stage_calls(b, 6), first[6])
        assert b.prove(trace, air, pub) == proof
