"""LSP_AIR_PROGRAM on the GPU: the program-capable instantiations of the
quotient and check kernels (k_air_prog.hpp).  The built-in configs restated as
programs must give the built-in descriptor's proof, byte for byte -- which the
C oracle pins; AIRs the oracle does not know are held to the big-integer
evaluator of tests/air_program_ref.py and to the host verifier."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import air_program_fuzz as F  # noqa: E402
import air_program_ref as A  # noqa: E402
import check_constraints_ref as ref  # noqa: E402
from linea_stark_prover_amd.air import lower, permutation_air  # noqa: E402
from linea_stark_prover_amd.field import GENERATOR, MODULUS, from_mont, to_mont, two_adic_generator  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)
R = MODULUS


def _pub(p):
    return np.concatenate([np.array(p.alpha, np.uint64).reshape(1, 4), np.array(p.delta, np.uint64).reshape(1, 4)])


@pytest.fixture(scope="module")
def shapes(gpu_ctx, oracle_lib):
    """name -> (trace, air, pub, the C oracle's proof), made once"""
    from linea_stark_prover_amd import prover as P
    p = oracle_lib.setup()
    pub = _pub(p)
    a, d = pub[0:1], pub[1:2]
    cache = {}

    def get(name):
        if name not in cache:
            if name.startswith("perm"):
                _, ncols, log_n = name.split("_")
                tr = P.gen_permutation_trace(int(log_n), int(ncols), a, d)
                air = permutation_air(int(ncols))
            elif name == "mixed_7":
                tr, air = P.gen_wide_trace(7, a, d, **ref.MIXED)
            else:
                assert name == "wide_8"
                tr, air = P.gen_wide_trace(8, a, d)
            tr = np.ascontiguousarray(tr)
            exp = oracle_lib.prove(p, tr.ctypes.data, tr.shape[0], tr.shape[1],
                                   oracle_lib.air_desc(ref.oracle_cfgs(air)))
            cache[name] = (tr, air, pub, exp)
        return cache[name]
    return get


# ---------------------------------------------------------- proof identity
@pytest.mark.parametrize("early", ["0", "1"])
@pytest.mark.parametrize("name", ["perm_3_2", "perm_3_5", "perm_3_8", "perm_3_10", "perm_6_6", "mixed_7", "wide_8"])
def test_lowered_proof_is_the_built_in_proof(gpu_ctx, shapes, monkeypatch, name, early):
    monkeypatch.setenv("LSP_QUOTIENT_EARLY", early)
    tr, air, pub, exp = shapes(name)
    got = gpu_ctx.prove(tr, lower(air), pub)
    assert got == exp
    assert gpu_ctx.prove(tr, air, pub) == exp
    assert gpu_ctx.verify(got, lower(air), pub) and gpu_ctx.verify(got, air, pub)


@pytest.mark.parametrize("early", ["0", "1"])
def test_mixed_descriptors(gpu_ctx, shapes, monkeypatch, early):
    """some configs lowered, some not: lookups as programs beside built-in
    permutations, and the other way round"""
    monkeypatch.setenv("LSP_QUOTIENT_EARLY", early)
    tr, air, pub, exp = shapes("mixed_7")
    for which in ({0}, {1, 2}, {0, 3}, {3}):
        assert gpu_ctx.prove(tr, lower(air, which), pub) == exp


@pytest.mark.parametrize("name,npoints", [("perm_3_2", 16), ("perm_3_8", 1024)])
def test_quotient_values_equal_the_built_in(gpu_ctx, shapes, name, npoints):
    """h = 2^2: a partial wave; h = 2^8: 1024 points, several blocks"""
    tr, air, pub, _ = shapes(name)
    h = tr.shape[0]
    lde = gpu_ctx.coset_lde_batch(tr, gpu_ctx.config.log_blowup, to_mont([GENERATOR]))
    alpha = to_mont([0x1234567 * 0x89abcdef + 5])
    exp = gpu_ctx.quotient_values(lde, h, air, pub, alpha)
    got = gpu_ctx.quotient_values(lde, h, lower(air), pub, alpha)
    assert got.shape[0] == npoints and np.array_equal(got, exp)


# ---------------------------------------------------------------- new AIRs
def _new(name, h):
    if name == "fibonacci":
        rows, extra = A.fibonacci_rows(h)
        return A.fibonacci_air(), rows, extra, 0
    d = int(name[4:])
    rows, extra = A.sbox_rows(h, d)
    return A.sbox_air(d), rows, extra, {5: 2, 9: 3}[d]


def _pubs(gpu_ctx, extra):
    a, d, _ = gpu_ctx.config.seeded()
    pubi = from_mont(np.concatenate([a, d])) + list(extra)
    return pubi, to_mont(pubi)


@pytest.mark.parametrize("log_h", [4, 9])
@pytest.mark.parametrize("name", ["fibonacci", "sbox5", "sbox9"])
def test_new_air_proves_and_verifies(gpu_ctx, name, log_h):
    from linea_stark_prover_amd import _lib as L
    import ctypes
    air, rows, extra, log_q = _new(name, 1 << log_h)
    desc = (ctypes.c_int32 * len(air.descriptor()))(*air.descriptor())
    lq = ctypes.c_uint32()
    L.check(L.lib().lsp_log_quotient_degree(desc, len(desc), gpu_ctx.config.public_degree, ctypes.byref(lq)))
    assert lq.value == log_q
    pubi, pub = _pubs(gpu_ctx, extra)
    tr = A.rows_to_trace(rows)
    proof = gpu_ctx.prove(tr, air, pub)
    assert gpu_ctx.verify(proof, air, pub)
    assert gpu_ctx.prove(tr, air, pub) == proof  # the same bytes twice
    # a changed public value, a flipped opened value (trace_local[0] follows the
    # 32-byte header and the two roots), another AIR
    bad = list(pubi)
    bad[2] = (bad[2] + 1) % R
    assert not gpu_ctx.verify(proof, air, to_mont(bad))
    flipped = bytearray(proof)
    flipped[32 + 64 + 3] ^= 0x10
    assert not gpu_ctx.verify(bytes(flipped), air, pub)
    other = A.sbox_air(9) if name == "sbox5" else A.sbox_air(5) if name == "sbox9" else A.slotless_air()
    assert not gpu_ctx.verify(proof, other, pub)


def _poly_evals(rows, log_h, log_n):
    """column polynomials of the trace evaluated on GEN * <w_N>, natural order"""
    h, N, w = 1 << log_h, 1 << log_n, len(rows[0])
    wh, wn = two_adic_generator(log_h), two_adic_generator(log_n)
    hinv = pow(h, R - 2, R)
    whinv = pow(wh, R - 2, R)
    coef = [[sum(rows[i][c] * pow(whinv, i * k, R) for i in range(h)) * hinv % R for k in range(h)]
            for c in range(w)]
    out = []
    for n in range(N):
        x = GENERATOR * pow(wn, n, R) % R
        out.append([sum(cf[k] * pow(x, k, R) for k in range(h)) % R for cf in coef])
    return out


def _brev(x, bits):
    return int(format(x, f"0{bits}b")[::-1], 2) if bits else 0


@pytest.mark.parametrize("name", ["fibonacci", "sbox5", "sbox9"])
def test_new_air_quotient_values_equal_the_evaluator(gpu_ctx, name):
    """h = 2^4: every point of the quotient domain against the big-integer
    evaluator folded by alpha and divided by Z_H"""
    log_h, lb = 4, gpu_ctx.config.log_blowup
    h, N = 1 << log_h, 1 << (log_h + lb)
    air, rows, extra, log_q = _new(name, h)
    pubi, pub = _pubs(gpu_ctx, extra)
    ev = _poly_evals(rows, log_h, log_h + lb)
    lde = np.zeros((N, len(rows[0]), 4), np.uint64)
    for n in range(N):
        lde[_brev(n, log_h + lb)] = to_mont(ev[n])
    alpha = 0xabcdef0123456789 * 0x1000193 + 11
    got = from_mont(gpu_ctx.quotient_values(lde, h, air, pub, to_mont([alpha])))
    Q = h << log_q
    assert len(got) == Q
    exp = F.quotient_ref(air, ev, h, log_q, pubi, alpha)
    for i in range(Q):
        assert got[i] == exp[i], (name, i)


@pytest.mark.parametrize("log_h", [3, 9])
@pytest.mark.parametrize("name", ["fibonacci", "sbox5", "sbox9"])
def test_new_air_check_equals_the_host_twin(gpu_ctx, name, log_h):
    """h = 2^3: a partial wave; 2^9: two blocks"""
    from linea_stark_prover_amd import prover as P
    h = 1 << log_h
    air, rows, extra, _ = _new(name, h)
    pubi, pub = _pubs(gpu_ctx, extra)
    host = P.Context(gpu_ctx.config, device=-1)
    try:
        for cells in ([], [(0, 0)], [(h - 1, 0), (h // 2, len(rows[0]) - 1), (1, 0)]):
            rr = [list(x) for x in rows]
            for r_, c in cells:
                rr[r_][c] = (rr[r_][c] + 1 + r_) % R
            tr = A.rows_to_trace(rr)
            exp = A.report(air, rr, pubi, 16)
            assert exp["ok"] == (not cells)
            g = gpu_ctx.check_constraints(tr, air, pub)
            assert ref.as_dict(g) == ref.as_dict(host.check_constraints(tr, air, pub)) == exp
    finally:
        host.close()


def test_lowered_check_equals_the_built_in(gpu_ctx, shapes):
    tr, air, pub, _ = shapes("mixed_7")
    rows = ref.ints(tr)
    alpha, delta = ref.pub_ints(pub)
    low = lower(air, {0, 3})
    assert gpu_ctx.check_constraints(tr, low, pub).ok
    for cls in ("lookup.a", "lookup.occurrences[1]", "perm.check", "perm.b"):
        t, rr = ref.tamper(tr, rows, 77, ref.column_classes(air)[cls])
        exp = ref.oracle_report(air, rr, alpha, delta, 64)
        for x in (low, lower(air)):
            assert ref.as_dict(gpu_ctx.check_constraints(t, x, pub, max_violations=64)) == exp


# ------------------------------------------------- slot and size pressure
def _pressure_cases():
    out = []
    for n in (8, 16):
        rows, extra = A.pressure_rows(64, n)
        out.append((f"slots{n}", A.pressure_air(n), rows, extra))
    air, k = A.long_air(2000)
    rows, extra = A.long_rows(64, k)
    out.append(("ops2000", air, rows, extra))
    out.append(("slots0", A.slotless_air(), [[i + 1, 0] for i in range(64)], []))
    return out


@pytest.mark.parametrize("name,air,rows,extra", _pressure_cases(), ids=[c[0] for c in _pressure_cases()])
def test_slot_and_size_pressure(gpu_ctx, name, air, rows, extra):
    cfg = air.configs[0]
    assert {"slots8": cfg.nslots == 8, "slots16": cfg.nslots == 16, "slots0": cfg.nslots == 0,
            "ops2000": len(cfg.ops) == 2000}[name]
    pubi, pub = _pubs(gpu_ctx, extra)
    tr = A.rows_to_trace(rows)
    assert A.report(air, rows, pubi, 4)["ok"]
    assert ref.as_dict(gpu_ctx.check_constraints(tr, air, pub)) == A.report(air, rows, pubi, 16)
    proof = gpu_ctx.prove(tr, air, pub)
    assert gpu_ctx.verify(proof, air, pub)
    # a broken cell: the check names it as the evaluator does
    rr = [list(x) for x in rows]
    rr[37][len(rr[0]) - 1] = (rr[37][len(rr[0]) - 1] + 5) % R
    exp = A.report(air, rr, pubi, 16)
    assert not exp["ok"]
    assert ref.as_dict(gpu_ctx.check_constraints(A.rows_to_trace(rr), air, pub)) == exp


def test_degree_ten_exceeds_the_blowup(gpu_ctx):
    from linea_stark_prover_amd import _lib as L
    air = A.sbox_air(10)
    rows, extra = A.sbox_rows(16, 10)
    _, pub = _pubs(gpu_ctx, extra)
    tr = A.rows_to_trace(rows)
    with pytest.raises(L.LspError, match="quotient degree exceeds the blowup") as e:
        gpu_ctx.prove(tr, air, pub)
    assert e.value.code == L.LSP_E_ARG
    lde = np.zeros((16 << gpu_ctx.config.log_blowup, 1, 4), np.uint64)
    with pytest.raises(L.LspError, match="quotient degree exceeds the blowup"):
        gpu_ctx.quotient_values(lde, 16, air, pub, to_mont([3]))


# ------------------------------------------------------------ virtual ranks
@pytest.mark.parametrize("G", [2, 8])
def test_virtual_ranks(gpu_ctx, shapes, G):
    from linea_stark_prover_amd.prover import Context, ProverGroup
    tr, air, pub, exp = shapes("perm_3_10")
    grp = ProverGroup([Context(gpu_ctx.config) for _ in range(G)])
    try:
        assert grp.prove(tr, lower(air), pub) == exp
        for name in ("fibonacci", "sbox5"):
            nair, rows, extra, _ = _new(name, 1 << 10)
            _, npub = _pubs(gpu_ctx, extra)
            t = A.rows_to_trace(rows)
            single = gpu_ctx.prove(t, nair, npub)
            assert gpu_ctx.verify(single, nair, npub)
            assert grp.prove(t, nair, npub) == single
    finally:
        grp.close()


# ------------------------------------------------------- debug-bounds build
CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import air_program_ref as A
from linea_stark_prover_amd import _lib as L
from linea_stark_prover_amd.air import lower, permutation_air
from linea_stark_prover_amd.field import from_mont, to_mont
from linea_stark_prover_amd.prover import Context, StarkConfig, gen_permutation_trace
assert b"debug-bounds" in L.lib().lsp_version()
with Context(StarkConfig()) as ctx:
    a, d, _ = ctx.config.seeded()
    pub = np.concatenate([a, d])
    tr = gen_permutation_trace(8, 3, a, d)
    got = ctx.prove(tr, lower(permutation_air(3)), pub)
    assert got == ctx.prove(tr, permutation_air(3), pub)
    air = A.pressure_air(16)
    rows, extra = A.pressure_rows(256, 16)
    p2 = to_mont(from_mont(pub) + extra)
    t = A.rows_to_trace(rows)
    assert ctx.check_constraints(t, air, p2).ok
    assert ctx.verify(ctx.prove(t, air, p2), air, p2)
    rows[9][3] += 1
    assert ctx.check_constraints(A.rows_to_trace(rows), air, p2).first == (8, 0)
print("debug-bounds ok")
'''


def test_debug_bounds_build_reports_no_failed_check():
    from linea_stark_prover_amd import build as B
    assert os.path.exists(B.DBG_LIB), "liblsp_hip_dbg.so not built (python -m linea_stark_prover_amd.build --debug-bounds)"
    env = dict(os.environ, LSP_LIB=B.DBG_LIB)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "debug-bounds ok" in r.stdout
