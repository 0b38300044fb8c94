"""The corners of the parameter domain lsp_ctx_create admits (include/lsp.h
lsp_params), as one table both tests/test_config_lattice.py (CPU: C oracle ->
host verifier) and tests/test_gpu_config_lattice.py (device proof == oracle
proof) walk.  No tests here.

A point is a trace size of the permutation AIR, the StarkConfig switches that
differ from the defaults, and what must happen: PROOF (a proof byte-identical
to the C oracle's) or a refusal, named by the error code and a piece of its
message.  `env` is set around the device proof only (the oracle's bytes do not
depend on where a round runs)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

PROOF = "proof"
PERM_KEYS = ("sbox_degree", "rounds_f", "rounds_p")
FRI_KEYS = ("log_blowup", "log_final_poly_len", "num_queries", "proof_of_work_bits", "sample_bits_montgomery")
# the C oracle's lo_params holds this many rounds (oracle/lsp_oracle.h); the context admits (64, 256)
ORACLE_MAX_ROUNDS = (16, 64)
HEIGHT_RULE = "an LDE height below 2 \\* 2\\^\\(log_blowup \\+ log_final_poly_len\\)"


@dataclass(frozen=True)
class Point:
    id: str
    log_n: int
    ncols: int
    cfg: tuple                      # sorted (key, value) pairs of StarkConfig
    expect: str = PROOF             # PROOF, or "LSP_E_xxx:<regex of the message>"
    env: tuple = ()                 # (name, value) pairs for the device proof
    ranks: int = 1                  # > 1: also proved by a group of that many virtual ranks

    @property
    def kw(self) -> dict:
        return dict(self.cfg)

    def part(self, keys) -> dict:
        return {k: v for k, v in self.cfg if k in keys}

    @property
    def public_degree(self) -> int:
        return self.kw.get("public_degree", 1)

    @property
    def log_q(self) -> int:
        """log2 of the permutation AIR's quotient chunks (tests/test_host.py holds it to the oracle)"""
        return (3 if self.ncols == 6 else 2) - (1 - self.public_degree)

    @property
    def lfp(self) -> int:
        return self.kw.get("log_final_poly_len", 0)

    def proof_key(self):
        """points with one key have one proof (they differ in env / ranks only)"""
        return (self.log_n, self.ncols, self.cfg)


def P(id, log_n, ncols, expect=PROOF, env=(), ranks=1, **cfg):
    assert ncols in (3, 6)
    return Point(id, log_n, ncols, tuple(sorted(cfg.items())), expect, tuple(sorted(dict(env).items())), ranks)


TAIL0 = {"LSP_FRI_HOST_TAIL": "0"}
SHARD = {"LSP_FRI_SHARD_MIN": "2"}

# Sizes: Merkle levels of <= 1024 digests and FRI rounds of <= 2048 leaves run on
# the host, so a point that is about a device path has 2^12 LDE rows or more.
BLOWUP = [
    P("blowup1-2^12", 12, 3, log_blowup=1, public_degree=0),      # 2 coset blocks, log_q = 1
    P("blowup1-2^1", 1, 3, log_blowup=1, public_degree=0),        # N = 4
    P("blowup1-pubdeg1-refused", 6, 3, "LSP_E_ARG:exceeds the blowup", log_blowup=1),
    P("blowup5-2^8", 8, 6, log_blowup=5),                         # 32 coset blocks
    P("blowup8-2^5", 5, 6, log_blowup=8),                         # 256 coset blocks, log_q = 3
    P("blowup8-2^1", 1, 6, log_blowup=8),
]
FINAL_POLY = [
    P("lfp8-one-round", 9, 3, log_final_poly_len=8),              # the boundary: log2(h) = lfp + 1
    P("lfp8-one-round-device", 9, 3, env=TAIL0, log_final_poly_len=8),
    P("lfp8-two-rounds", 10, 3, log_final_poly_len=8),
    P("lfp8-two-rounds-device", 10, 3, env=TAIL0, log_final_poly_len=8),
    P("lfp4-blowup1", 5, 3, log_blowup=1, log_final_poly_len=4, public_degree=0),
    P("lfp3-blowup8", 4, 3, log_blowup=8, log_final_poly_len=3),
    P("lfp3-no-round-refused", 3, 3, "LSP_E_SIZE:" + HEIGHT_RULE, ranks=2, log_final_poly_len=3),
    P("lfp3-below-refused", 2, 3, "LSP_E_SIZE:" + HEIGHT_RULE, ranks=2, log_final_poly_len=3),
]
QUERIES = [
    P("queries1024-2^1", 1, 3, num_queries=1024),                 # 16 LDE rows, each opened many times
    P("queries1024-2^9", 9, 3, num_queries=1024),
    P("queries1-2^9", 9, 3, num_queries=1),
]
# The oracle grinds on the CPU, one thread, 2^bits tries expected.  16 bits, the
# most this table takes, cost it 3.2 s (canonical bits) and 1.7 s (Montgomery
# bits) on these seeds; 17 would double that.
GRINDING = [
    P("pow16", 9, 3, proof_of_work_bits=16),
    P("pow16-montgomery-bits", 9, 3, proof_of_work_bits=16, sample_bits_montgomery=True),
]
# 2^13 rows: N = 2^16, so leaves and levels cross the one-lane, pair, quad and row forms
ROUNDS = [
    P("rounds2,0", 13, 3, rounds_f=2, rounds_p=0),
    P("rounds2,1", 13, 3, rounds_f=2, rounds_p=1),
    P("rounds16,64", 13, 3, rounds_f=16, rounds_p=64),            # the C oracle's capacity
    P("sbox17-rounds4,3", 9, 3, sbox_degree=17, rounds_f=4, rounds_p=3, log_blowup=2, log_final_poly_len=1,
      proof_of_work_bits=8),
]
# group proof == single proof == oracle proof, every FRI round sharded (LSP_FRI_SHARD_MIN=2)
SHARDED = [
    P("shard-blowup1-G2", 9, 3, env=SHARD, ranks=2, log_blowup=1, public_degree=0),
    P("shard-blowup1-G4", 9, 3, env=SHARD, ranks=4, log_blowup=1, public_degree=0),   # more ranks than cosets
    P("shard-blowup2-lfp2-G4", 9, 3, env=SHARD, ranks=4, log_blowup=2, log_final_poly_len=2),  # final vector sharded
    P("shard-blowup5-lfp3-G8", 7, 3, env=SHARD, ranks=8, log_blowup=5, log_final_poly_len=3),
]
POINTS = BLOWUP + FINAL_POLY + QUERIES + GRINDING + ROUNDS + SHARDED
assert len({p.id for p in POINTS}) == len(POINTS)

# Beyond the C oracle's capacity there is no whole-proof reference: the device is
# held per operation to the context's host Poseidon2, and that to big integers
# (tests/test_config_lattice.py), at these and at the smallest round counts.
BEYOND_ORACLE = [dict(rounds_f=64, rounds_p=256), dict(sbox_degree=17, rounds_f=64, rounds_p=255),
                 dict(rounds_f=8, rounds_p=256)]
HOST_POSEIDON2 = [dict(rounds_f=2, rounds_p=0), dict(rounds_f=2, rounds_p=1)] + BEYOND_ORACLE


def ids(cases):
    return [",".join(f"{k}={v}" for k, v in c.items()) for c in cases]


# --------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def _oracle_inputs(perm: tuple, log_n: int, ncols: int):
    from oracle import cref
    p = cref.setup(**dict(perm))
    tb, w = cref.gen_perm_trace(p, log_n, ncols)
    trace = np.frombuffer(tb.raw, dtype=np.uint64).reshape(1 << log_n, w, 4).copy()
    pub = np.concatenate([np.array(p.alpha, np.uint64).reshape(1, 4), np.array(p.delta, np.uint64).reshape(1, 4)])
    trace.setflags(write=False)
    pub.setflags(write=False)
    return p, trace, pub


def inputs(pt: Point):
    """(oracle params, trace (h, w, 4), public values (2, 4)) of a point; shared, read-only"""
    return _oracle_inputs(tuple(sorted(pt.part(PERM_KEYS).items())), pt.log_n, pt.ncols)


def oracle_fri(pt: Point):
    from oracle import cref
    from oracle import pyoracle as O
    return cref.fri_params(O.FriParams(**pt.part(FRI_KEYS)))


_proofs = {}


def oracle_proof(pt: Point) -> bytes:
    """the C oracle's proof of a point, computed once per distinct (size, config);
    raises RuntimeError where the oracle refuses"""
    from oracle import cref
    key = pt.proof_key()
    if key not in _proofs:
        p, trace, _ = inputs(pt)
        _proofs[key] = cref.prove(p, trace.ctypes.data, 1 << pt.log_n, trace.shape[1], cref.perm_air(pt.ncols),
                                  fri=oracle_fri(pt), public_degree=pt.public_degree, nthreads=16)
    return _proofs[key]


def stark_config(pt: Point):
    from linea_stark_prover_amd.prover import StarkConfig
    return StarkConfig(**pt.kw)


def final_poly_offset(pt: Point, k: int) -> int:
    """byte offset of final-polynomial coefficient k in an LSPPRF02 proof:
    magic, 6 header words, 2 roots, the opened values, one root per FRI round"""
    nr = pt.log_n - pt.lfp
    return 8 + 24 + 64 + 32 * (2 * (2 * pt.ncols + 2) + (1 << pt.log_q)) + 32 * nr + 32 * k


def flip_last_final_coefficient(pt: Point, proof: bytes) -> bytes:
    bad = bytearray(proof)
    bad[final_poly_offset(pt, (1 << pt.lfp) - 1)] ^= 1
    return bytes(bad)
