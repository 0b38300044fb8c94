"""The corners of the admitted parameter domain on the CPU (tests/config_cases.py).

Every point's C-oracle proof is accepted by the host verifier (and, with a
one-coefficient final polynomial, by the oracle's own), and a flipped byte in
the last final-polynomial coefficient is rejected.  The height rule
log2(h) > log_final_poly_len holds on every side: the oracles refuse to prove,
the verifier rejects a zero-round header at check 4.  The host Poseidon2 -- the
device's reference above the C oracle's (16, 64) rounds -- is held to big
integers at the smallest and largest admitted round counts."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import config_cases as C  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

PROVED = {p.proof_key(): p for p in C.POINTS if p.expect == C.PROOF}.values()  # one per distinct proof


def _host_ctx(pt):
    from linea_stark_prover_amd.prover import Context
    return Context(C.stark_config(pt), device=-1)


def _reject_check(ctx, proof, air, pub):
    from linea_stark_prover_amd import _lib as L
    assert not ctx.verify(proof, air, pub)
    msg = L.lib().lsp_last_error(None).decode()
    assert msg.startswith("proof rejected at check "), msg
    return int(msg.rsplit(" ", 1)[1])


@pytest.mark.parametrize("pt", PROVED, ids=lambda p: p.id)
def test_oracle_proof_verifies(oracle_lib, product_lib, pt):
    from linea_stark_prover_amd.air import permutation_air
    p, _, pub = C.inputs(pt)
    proof = C.oracle_proof(pt)
    air = permutation_air(pt.ncols)
    with _host_ctx(pt) as ctx:
        assert ctx.verify(proof, air, pub)
        # the header says what the point is about: rounds above the final polynomial, its length, the queries
        log_h, log_q, _, nq, nr, nf = struct.unpack_from("<6I", proof, 8)
        assert (log_h, log_q, nq, nr, nf) == (pt.log_n, pt.log_q, pt.kw.get("num_queries", 33), pt.log_n - pt.lfp,
                                              1 << pt.lfp)
        assert nr >= 1
        assert not ctx.verify(C.flip_last_final_coefficient(pt, proof), air, pub)
    if pt.lfp == 0:  # the C oracle's verifier reads a 1-coefficient final polynomial only
        assert oracle_lib.verify(p, proof, oracle_lib.perm_air(pt.ncols), fri=C.oracle_fri(pt),
                                 public_degree=pt.public_degree) == 0


@pytest.mark.parametrize("pt", [p for p in C.POINTS if p.expect != C.PROOF], ids=lambda p: p.id)
def test_refused_points_are_refused_by_the_oracle_too(oracle_lib, pt):
    with pytest.raises(RuntimeError, match="lo_prove failed"):
        C.oracle_proof(pt)


# ---------------------------------------------------------------- height rule
BOUNDARY = [(lfp, lb, d) for lfp in (1, 3, 8) for lb in (1, 3) for d in (0, 1)]  # log2(h) = lfp - d


def _boundary_point(lfp, lb, log_n):
    return C.P(f"lfp{lfp}-blowup{lb}-2^{log_n}", log_n, 3, log_blowup=lb, log_final_poly_len=lfp,
               public_degree=0 if lb == 1 else 1, num_queries=2)


@pytest.mark.parametrize("lfp,lb,d", BOUNDARY)
def test_no_fri_round_oracle_refuses(oracle_lib, lfp, lb, d):
    """log2(h) == lfp and lfp - 1: lo_prove returns an error (h = 1 is no trace at all)"""
    log_n = lfp - d
    pt = _boundary_point(lfp, lb, log_n)
    p = oracle_lib.setup()
    tb, w = oracle_lib.gen_perm_trace(p, max(log_n, 1), 3)
    with pytest.raises(RuntimeError, match="lo_prove failed: -2" if log_n == 0 else "lo_prove failed: -5"):
        oracle_lib.prove(p, tb, 1 << log_n, w, oracle_lib.perm_air(3), fri=C.oracle_fri(pt),
                         public_degree=pt.public_degree)
    # one row more and it proves
    if d == 0:
        up = _boundary_point(lfp, lb, lfp + 1)
        assert C.oracle_proof(up)[:8] == b"LSPPRF02"


def test_no_fri_round_pyoracle_refuses():
    s = O.setup_from_seed()
    cfgs, cols = O.synthetic_perm_trace(1, 3, s.alpha, s.delta, O.DEFAULT_SEED)
    with pytest.raises(AssertionError, match="log_final_poly_len"):
        O.prove(cfgs, O.columns_to_rows(cols), [s.alpha, s.delta], s.perm, O.FriParams(log_final_poly_len=1))


@pytest.mark.parametrize("lfp,lb,d", BOUNDARY)
def test_zero_round_proof_rejected_at_check_4(oracle_lib, product_lib, lfp, lb, d):
    """A one-round proof (log2(h) = lfp + 1) whose header is rewritten to the
    zero-round shape -- log_h = lfp - d, no FRI round, the same final-polynomial
    length -- is what a prover without the height rule would hand out: check 4
    rejects it before the round count is computed.  (log_h = 0 is no trace and
    falls at check 3, which comes first.)"""
    from linea_stark_prover_amd.air import permutation_air
    one = _boundary_point(lfp, lb, lfp + 1)
    proof = C.oracle_proof(one)
    _, _, pub = C.inputs(one)
    air = permutation_air(3)
    with _host_ctx(one) as ctx:
        assert ctx.verify(proof, air, pub)
        log_h, log_q, w, nq, nr, nf = struct.unpack_from("<6I", proof, 8)
        assert (log_h, nr, nf) == (lfp + 1, 1, 1 << lfp)
        bad = proof[:8] + struct.pack("<6I", lfp - d, log_q, w, nq, 0, nf) + proof[32:]
        assert _reject_check(ctx, bad, air, pub) == (3 if lfp - d == 0 else 4)
        # the round count alone (the header still says lfp + 1 rows) is check 4 as before
        assert _reject_check(ctx, proof[:8] + struct.pack("<6I", log_h, log_q, w, nq, 0, nf) + proof[32:], air,
                             pub) == 4


# ------------------------------------------------------- oracle capacity
@pytest.mark.parametrize("rf,rp", [(64, 256), (18, 64), (16, 65)])
def test_oracle_refuses_rounds_beyond_its_capacity(oracle_lib, rf, rp):
    with pytest.raises(ValueError, match="capacity"):
        oracle_lib.setup(rounds_f=rf, rounds_p=rp)
    # a hand-filled lo_params is refused by lo_prove as well
    p = oracle_lib.setup()
    tb, w = oracle_lib.gen_perm_trace(p, 2, 3)
    p.rounds_f, p.rounds_p = rf, rp
    with pytest.raises(RuntimeError, match="lo_prove failed: -4"):
        oracle_lib.prove(p, tb, 4, w, oracle_lib.perm_air(3))
    assert oracle_lib.verify(p, b"LSPPRF02" + bytes(64), oracle_lib.perm_air(3)) == -4
    assert oracle_lib.setup(rounds_f=C.ORACLE_MAX_ROUNDS[0], rounds_p=C.ORACLE_MAX_ROUNDS[1]).rounds_p == 64


# ------------------------------------------------------- host Poseidon2
@pytest.mark.parametrize("perm", C.HOST_POSEIDON2, ids=C.ids(C.HOST_POSEIDON2))
def test_host_poseidon2_matches_big_integers(product_lib, perm):
    """lsp_host_compress_batch and lsp_host_hash_rows against pyoracle at the
    smallest and largest admitted round counts; 1, 9 and 17 states cross the
    8- and 16-lane IFMA paths and leave a scalar remainder"""
    from linea_stark_prover_amd.field import from_mont, to_mont
    from linea_stark_prover_amd.prover import Context, StarkConfig
    pp = O.setup_from_seed(**perm).perm
    rng = np.random.default_rng(sum(perm.values()))
    edge = [0, 1, O.P - 1, O.P - 2]
    with Context(StarkConfig(**perm), device=-1) as ctx:
        for n in (1, 9, 17):
            vals = [int.from_bytes(rng.bytes(32), "little") % O.P for _ in range(2 * n)]
            vals[:len(edge)] = edge[:2 * n]
            pairs, out = to_mont(vals), np.zeros((n, 4), np.uint64)
            assert product_lib.lsp_host_compress_batch(ctx.h, ctypes.c_void_p(pairs.ctypes.data), n,
                                                       ctypes.c_void_p(out.ctypes.data)) == 0
            assert from_mont(out) == [O.compress(vals[2 * i], vals[2 * i + 1], pp) for i in range(n)], f"compress {n}"
            for w in (1, 2, 3, 8):
                vals = [int.from_bytes(rng.bytes(32), "little") % O.P for _ in range(n * w)]
                vals[:len(edge)] = edge[:n * w]
                rows, out = to_mont(vals), np.zeros((n, 4), np.uint64)
                assert product_lib.lsp_host_hash_rows(ctx.h, ctypes.c_void_p(rows.ctypes.data), n, w,
                                                      ctypes.c_void_p(out.ctypes.data)) == 0
                assert from_mont(out) == [O.hash_iter(vals[i * w:(i + 1) * w], pp) for i in range(n)], \
                    f"hash_rows {n} x {w}"
