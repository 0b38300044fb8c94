"""The corners of the admitted parameter domain on the device
(tests/config_cases.py; tests/test_config_lattice.py is the CPU side).

Every point of the table is either a proof byte-identical to the C oracle's,
which the context's verifier accepts, or an asserted refusal.  Each point has a
context of its own, the permutation AIR and the oracle's trace.  Above the C
oracle's (16, 64) rounds no whole-proof reference exists: there the device is
held per operation to the context's host Poseidon2, which the CPU file holds
to big integers at the same round counts."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import config_cases as C  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


def _group_prove(cfg, G, trace, air, pub):
    from linea_stark_prover_amd.prover import Context, ProverGroup
    ctxs = [Context(cfg) for _ in range(G)]
    grp = ProverGroup(ctxs)
    try:
        return grp.prove(trace, air, pub)
    finally:
        grp.close()
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("pt", C.POINTS, ids=lambda p: p.id)
def test_lattice_point(oracle_lib, product_lib, monkeypatch, pt):
    from linea_stark_prover_amd import _lib as L
    from linea_stark_prover_amd.air import permutation_air
    from linea_stark_prover_amd.prover import Context
    for k, v in pt.env:
        monkeypatch.setenv(k, v)
    _, trace, pub = C.inputs(pt)
    air = permutation_air(pt.ncols)
    cfg = C.stark_config(pt)
    if pt.expect != C.PROOF:
        code, msg = pt.expect.split(":", 1)
        with Context(cfg) as ctx, pytest.raises(L.LspError, match=msg) as e:
            ctx.prove(trace, air, pub)
        assert e.value.code == getattr(L, code)
        if pt.ranks > 1:
            with pytest.raises(L.LspError, match=msg) as e:
                _group_prove(cfg, pt.ranks, trace, air, pub)
            assert e.value.code == getattr(L, code)
        return
    want = C.oracle_proof(pt)
    with Context(cfg) as ctx:
        got = ctx.prove(trace, air, pub)
        assert got == want
        assert ctx.verify(got, air, pub)
        assert not ctx.verify(C.flip_last_final_coefficient(pt, got), air, pub)
    if pt.ranks > 1:
        assert _group_prove(cfg, pt.ranks, trace, air, pub) == want


# ------------------------------------------- beyond the C oracle's capacity
def _rand_mont(rng, shape):
    """uniform 4-limb values below 2^252 < r: each is some element's Montgomery form"""
    a = rng.integers(0, 1 << 63, tuple(shape) + (4,), dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, tuple(shape) + (4,), dtype=np.uint64)
    a[..., 3] &= np.uint64((1 << 60) - 1)
    return a


def _edges():
    from linea_stark_prover_amd.field import to_mont
    return to_mont([0, 1, O.P - 1, O.P - 2, 2, O.P // 2])


def _host_hash_rows(lib, ctx, rows):
    out = np.zeros((rows.shape[0], 4), np.uint64)
    assert lib.lsp_host_hash_rows(ctx.h, ctypes.c_void_p(rows.ctypes.data), rows.shape[0], rows.shape[1],
                                  ctypes.c_void_p(out.ctypes.data)) == 0
    return out


def _host_compress(lib, ctx, layer):
    out = np.zeros((layer.shape[0] // 2, 4), np.uint64)
    assert lib.lsp_host_compress_batch(ctx.h, ctypes.c_void_p(layer.ctypes.data), out.shape[0],
                                       ctypes.c_void_p(out.ctypes.data)) == 0
    return out


@pytest.fixture(scope="module", params=C.BEYOND_ORACLE, ids=C.ids(C.BEYOND_ORACLE))
def big(request, product_lib):
    from linea_stark_prover_amd.prover import Context, StarkConfig
    cfg = StarkConfig(**request.param)
    with Context(cfg) as ctx:
        yield dict(ctx=ctx, cfg=cfg, perm=request.param, lib=product_lib)


# rows: 1001 takes the quad form, 20001 the lane-pair form, 33001 one state per lane
@pytest.mark.parametrize("w,ns", [(1, (1001, 33001)), (2, (20001, 33001)), (3, (1001, 20001, 33001)),
                                  (8, (1001, 20001))])
def test_hash_rows_beyond_oracle(big, w, ns):
    rng = np.random.default_rng(w)
    for n in ns:
        rows = _rand_mont(rng, (n, w))
        e = _edges()
        rows.reshape(-1, 4)[:len(e)] = e[:n * w]
        rows[-1, -1] = e[2]
        got = big["ctx"].hash_rows(rows)
        assert np.array_equal(got, _host_hash_rows(big["lib"], big["ctx"], rows)), f"{n} rows"


def test_merkle_layers_beyond_oracle(big, monkeypatch):
    """2^16 leaves with no host tree top: the levels cross the one-lane, pair,
    quad and row forms, each against the host compression of the level below"""
    from linea_stark_prover_amd.prover import MerkleTreeMmcs
    monkeypatch.setenv("LSP_HOST_TREE_TOP", "0")
    logh = 16
    rows = _rand_mont(np.random.default_rng(16), (1 << logh, 3))
    root, tree = MerkleTreeMmcs(big["ctx"]).commit([rows])
    below = tree.layer(0)
    assert np.array_equal(below, _host_hash_rows(big["lib"], big["ctx"], rows)), "leaves"
    for lv in range(1, logh + 1):
        layer = tree.layer(lv)
        assert np.array_equal(layer, _host_compress(big["lib"], big["ctx"], below)), f"layer {lv}"
        below = layer
    assert np.array_equal(root.reshape(4), below.reshape(4))


def test_permute_beyond_oracle(big):
    from linea_stark_prover_amd.field import from_mont, to_mont
    pp = O.setup_from_seed(**big["perm"]).perm
    rng = np.random.default_rng(64)
    vals = [int.from_bytes(rng.bytes(32), "little") % O.P for _ in range(3 * 64)]
    vals[:6] = [0, 0, 0, O.P - 1, O.P - 1, O.P - 1]
    got = from_mont(big["ctx"].poseidon2_permute(to_mont(vals).reshape(64, 3, 4)).reshape(-1, 4))
    assert got == [x for i in range(64) for x in O.permute(vals[3 * i:3 * i + 3], pp)]


def test_proof_beyond_oracle_verifies(big):
    from linea_stark_prover_amd.air import permutation_air
    from linea_stark_prover_amd.prover import gen_permutation_trace
    a, d, _ = big["cfg"].seeded()
    trace = gen_permutation_trace(9, 3, a, d)
    pub = np.concatenate([a, d])
    air = permutation_air(3)
    proof = big["ctx"].prove(trace, air, pub)
    assert big["ctx"].verify(proof, air, pub)
    pt = C.P("beyond", 9, 3, **big["perm"])
    assert not big["ctx"].verify(C.flip_last_final_coefficient(pt, proof), air, pub)
    bad = bytearray(proof)
    bad[len(proof) - 1] ^= 1  # the last sibling digest of the last query's last FRI path
    assert not big["ctx"].verify(bytes(bad), air, pub)
