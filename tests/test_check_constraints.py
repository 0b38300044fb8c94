"""check_constraints on the host-only context (CPU): p3-uni-stark's debug-build
check of the trace against the AIR (lsp_check_constraints' host twin, a plain
loop over Air::eval) against oracle/pyoracle.py eval_constraints called per row
with 0/1 selectors -- the whole report: summary, every count, every first row,
the detail list with values.  tests/test_gpu_check_constraints.py holds the
device kernel to the same oracle."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import check_constraints_ref as ref  # noqa: E402
from linea_stark_prover_amd.air import LineaAIR, permutation_air  # noqa: E402
from linea_stark_prover_amd.field import MODULUS, to_mont  # noqa: E402


@pytest.fixture(scope="module")
def env(product_lib):
    from linea_stark_prover_amd import _lib as L
    from linea_stark_prover_amd import prover as P
    ctx = P.Context(P.StarkConfig(), device=-1)
    a, d, _ = ctx.config.seeded()
    pub = np.concatenate([a, d])
    alpha, delta = ref.pub_ints(pub)
    cache = {}

    def traces(log_n):
        """(perm trace, perm air, mixed trace, mixed air) with their int rows, made once per size"""
        if log_n not in cache:
            tp = P.gen_permutation_trace(log_n, 3, a, d)
            tm, am = P.gen_wide_trace(log_n, a, d, **ref.MIXED)
            cache[log_n] = {"perm": (tp, permutation_air(3), ref.ints(tp)), "mixed": (tm, am, ref.ints(tm))}
        return cache[log_n]

    yield dict(L=L, P=P, ctx=ctx, pub=pub, alpha=alpha, delta=delta, a=a, d=d, traces=traces)
    ctx.close()


def _desc(air):
    d = air.descriptor()
    return (ctypes.c_int32 * len(d))(*d), len(d)


KINDS = {0: "b_inverse", 1: "a_inverse", 2: "first_row", 3: "transition", 4: "last_row"}


def test_num_constraints(env):
    L, P = env["L"], env["P"]
    wide_desc_air = P.gen_wide_trace(1, env["a"], env["d"])[1]
    mixed = env["traces"](1)["mixed"][1]
    for air, nperm, lookups in ((permutation_air(3), 1, []), (permutation_air(6), 1, []),
                                (wide_desc_air, 8, [2] * 4), (mixed, 2, [2] * 2)):
        desc, n = _desc(air)
        got = ctypes.c_uint32()
        L.check(L.lib().lsp_air_num_constraints(desc, n, ctypes.byref(got)))
        row = [0] * air.width
        assert got.value == len(ref.O.eval_constraints(ref.oracle_cfgs(air), row, row, 1, 1, 1, 1, 1))
        assert got.value == 4 * nperm + sum(4 + t for t in lookups) == len(air.constraint_names())


def test_constraint_names_match_constraint_info(env):
    L = env["L"]
    for air in (permutation_air(3), env["traces"](1)["mixed"][1]):
        desc, n = _desc(air)
        names = air.constraint_names()
        for j, name in enumerate(names):
            cfg, typ, kind, tab = ctypes.c_uint32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
            L.check(L.lib().lsp_air_constraint_info(desc, n, j, ctypes.byref(cfg), ctypes.byref(typ),
                                                    ctypes.byref(kind), ctypes.byref(tab)))
            t = "permutation" if typ.value == L.LSP_AIR_PERMUTATION else "lookup"
            k = KINDS[kind.value] + (f"[{tab.value}]" if tab.value >= 0 else "")
            assert f"cfg {cfg.value} {t}: {k}" == name
            assert (tab.value >= 0) == (t == "lookup" and kind.value == L.LSP_CONSTRAINT_B_INVERSE)
        assert L.lib().lsp_air_constraint_info(desc, n, len(names), None, None, None, None) == L.LSP_E_ARG
    assert names[2] == "cfg 0 lookup: b_inverse[1]" and names[-2] == "cfg 3 permutation: transition"


@pytest.mark.parametrize("log_n", [1, 6, 10])
@pytest.mark.parametrize("which", ["perm", "mixed"])
def test_valid_traces_hold(env, log_n, which):
    trace, air, rows = env["traces"](log_n)[which]
    exp = ref.oracle_report(air, rows, env["alpha"], env["delta"], 16)
    assert exp["ok"] and not any(exp["counts"])
    r = env["ctx"].check_constraints(trace, air, env["pub"])
    assert ref.as_dict(r) == exp
    assert r.ok and r.first is None and r.details == [] and r.first_rows == [None] * len(r.counts)
    assert "hold" in str(r)


def _classes():
    return ["perm.a", "perm.b", "perm.b_inverse", "perm.check", "lookup.a", "lookup.b[1]", "lookup.a_filter",
            "lookup.b_filter[1]", "lookup.a_inverses", "lookup.b_inverses[1]", "lookup.occurrences[1]",
            "lookup.check"]


@pytest.mark.parametrize("row", ["0", "1", "h-2", "h-1"])
@pytest.mark.parametrize("cls", _classes())
def test_one_tampered_cell(env, cls, row):
    h = 64
    trace, air, rows = env["traces"](6)["mixed"]
    r_ = {"0": 0, "1": 1, "h-2": h - 2, "h-1": h - 1}[row]
    col = ref.column_classes(air)[cls]
    t, rr = ref.tamper(trace, rows, r_, col)
    exp = ref.oracle_report(air, rr, env["alpha"], env["delta"], 64)
    # (a b_filter cell beside a zero multiplicity enters no constraint: the oracle says so too)
    assert not exp["ok"] or cls == "lookup.b_filter[1]"
    rep = env["ctx"].check_constraints(t, air, env["pub"], max_violations=64)
    assert ref.as_dict(rep) == exp
    if not exp["ok"]:
        assert str(rep).startswith(
            f"constraints had nonzero value on row {exp['first'][0]}: constraint {exp['first'][1]} ")


def test_selectors_at_the_ends(env):
    """row h-1's transition constraint stays silent while row 0's first-row
    constraint fires (and the last-row constraint fires on row h-1 only)"""
    h = 64
    trace, air, rows = env["traces"](6)["mixed"]
    names = air.constraint_names()
    for cls, cfg in (("perm.check", 3), ("lookup.check", 1)):
        col = ref.column_classes(air)[cls]
        kind = "permutation" if cls.startswith("perm") else "lookup"
        first, trans, last = (names.index(f"cfg {cfg} {kind}: {k}") for k in ("first_row", "transition", "last_row"))
        t, rr = ref.tamper(trace, rows, 0, col)
        rep = env["ctx"].check_constraints(t, air, env["pub"], max_violations=64)
        assert ref.as_dict(rep) == ref.oracle_report(air, rr, env["alpha"], env["delta"], 64)
        hit = {(v.row, v.index) for v in rep.details}
        assert (0, first) in hit and (0, trans) in hit and (h - 1, trans) not in hit
        assert rep.counts[first] == 1 and rep.first_rows[first] == 0 and rep.counts[last] == 0
        t, rr = ref.tamper(trace, rows, h - 1, col)
        rep = env["ctx"].check_constraints(t, air, env["pub"], max_violations=64)
        assert ref.as_dict(rep) == ref.oracle_report(air, rr, env["alpha"], env["delta"], 64)
        hit = {(v.row, v.index) for v in rep.details}
        assert (h - 1, last) in hit and (h - 2, trans) in hit and (h - 1, trans) not in hit
        assert rep.counts[first] == 0 and rep.counts[trans] == 1


def test_wrong_public_values_fail_every_inverse_on_every_row(env):
    trace, air, rows = env["traces"](6)["mixed"]
    h = len(rows)
    bad = to_mont([(env["alpha"] + 1) % MODULUS, (env["delta"] + 1) % MODULUS])
    exp = ref.oracle_report(air, rows, (env["alpha"] + 1) % MODULUS, (env["delta"] + 1) % MODULUS, 16)
    rep = env["ctx"].check_constraints(trace, air, bad)
    assert ref.as_dict(rep) == exp
    inv = [j for j, n in enumerate(rep.names) if "inverse" in n]
    assert len(inv) == 2 * 3 + 2 and all(rep.counts[j] == h for j in inv)
    assert rep.failed_rows == h and rep.first == (0, 0)


@pytest.mark.parametrize("cap", [0, 1, 5, 1000])
def test_max_violations(env, cap):
    trace, air, rows = env["traces"](6)["mixed"]
    cols = ref.column_classes(air)
    t, rr = trace, rows
    for r_, cls in ((40, "lookup.a_inverses"), (3, "perm.check"), (3, "lookup.b_inverses[1]"), (17, "perm.a")):
        t, rr = ref.tamper(t, rr, r_, cols[cls])
    exp = ref.oracle_report(air, rr, env["alpha"], env["delta"], cap)
    assert exp["violations"] > 5
    rep = env["ctx"].check_constraints(t, air, env["pub"], max_violations=cap)
    assert ref.as_dict(rep) == exp
    got = [(v.row, v.index) for v in rep.details]
    assert got == sorted(got) and len(got) == min(cap, exp["violations"])
    if cap:
        assert got[0] == rep.first


def test_argument_errors(env):
    L, ctx = env["L"], env["ctx"]
    trace, air, _ = env["traces"](6)["perm"]

    def code(*a, **k):
        with pytest.raises(L.LspError) as e:
            ctx.check_constraints(*a, **k)
        return e.value.code

    assert code(trace, permutation_air(4), env["pub"]) == L.LSP_E_ARG          # column ids 8, 9 >= w = 8
    assert code(trace[:48], air, env["pub"]) == L.LSP_E_ARG                    # 48 rows
    assert code(trace, air, env["pub"][:1]) == L.LSP_E_ARG                     # npub = 1
    assert code(trace, LineaAIR([]), env["pub"]) == L.LSP_E_ARG                # Air::parse
    # a host-only context has no device memory to check
    assert code(1 << 20, air, env["pub"], h=64, w=8) == L.LSP_E_STATE
    desc, n = _desc(air)
    s = L.LspCheckSummary()
    t = np.ascontiguousarray(trace)
    assert L.lib().lsp_check_constraints(ctx.h, t.ctypes.data, 64, 8, desc, n, env["pub"].ctypes.data, 2, 0,
                                         ctypes.byref(s), None, None, None, 0, None) == L.LSP_OK
    assert (s.failed_rows, s.violations, s.ncons) == (0, 0, 4) and s.first_row == 2 ** 64 - 1
    assert L.lib().lsp_check_constraints(ctx.h, t.ctypes.data, 64, 8, desc, n, env["pub"].ctypes.data, 2, 0,
                                         None, None, None, None, 0, None) == L.LSP_E_ARG
    assert L.lib().lsp_check_constraints(ctx.h, t.ctypes.data, 64, 8, desc, n, env["pub"].ctypes.data, 2, 0,
                                         ctypes.byref(s), None, None, None, 4, None) == L.LSP_E_ARG


def test_prove_check_raises_before_proving(env):
    P = env["P"]
    trace, air, rows = env["traces"](6)["perm"]
    t, rr = ref.tamper(trace, rows, 9, air.configs[0].check_id)
    exp = ref.oracle_report(air, rr, env["alpha"], env["delta"], 16)
    with pytest.raises(P.ConstraintError) as e:
        env["ctx"].prove(t, air, env["pub"], check=True)
    assert ref.as_dict(e.value.report) == exp and e.value.report.first == (8, 2)
    with pytest.raises(P.ConstraintError):
        P.prove(env["ctx"].config, air, t, env["pub"], ctx=env["ctx"], check=True)


# --- the device kernel's zero test (k_check.hip f29_is_zero_mod_r), as integers
def test_zero_test_bound():
    """Every value k_check tests left Q29::sub (f29_reduce_qt of f29_sub16) or
    f29_reduce: normalised limbs, < 2 r.  On such values "limbs all zero or
    equal to r's" is exactly "zero mod r" -- checked on differences of equal
    residues in different lazy representatives (minuend < 20 r, subtrahend
    < 16 r: the bounds of Q29::sub), where the reduced result is 0 or r, and on
    nonzero differences."""
    import test_f29_bounds as B

    def is_zero(o):
        return all(x == 0 for x in o) or o == B.P29

    def sub(av, bv):
        d = [x + B.L16[i] - y for i, (x, y) in enumerate(zip(B.limbs(av), B.limbs(bv)))]
        assert min(d) >= 0
        o = B.f29_reduce_qt(d)
        B.check_reduced(o, av - bv)
        return o

    rng = random.Random(29)
    seen = set()
    for _ in range(2000):
        x = rng.randrange(B.R)
        ka, kb = rng.randrange(20), rng.randrange(16)
        o = sub(x + ka * B.R, x + kb * B.R)
        assert is_zero(o)
        seen.add(B.val(o) // B.R)
        y = (x + 1 + rng.randrange(B.R - 1)) % B.R  # != x mod r
        assert not is_zero(sub(x + ka * B.R, y + kb * B.R))
        # a loaded cell: X * 2^5 of any word below 2^256 through f29_reduce
        wv = rng.randrange(1 << 256)
        o = B.f29_reduce(B.limbs(wv << 5))
        assert all(v <= B.MASK for v in o[:8]) and B.val(o) < 2 * B.R and B.val(o) % B.R == (wv << 5) % B.R
        assert is_zero(o) == (B.val(o) % B.R == 0)
    # a zero difference comes out as r (the 16 r of f29_sub16 is never wholly taken back) and a zero
    # cell as 0 (the lookup's last-row constraint tests a loaded cell): both representatives occur
    assert seen <= {0, 1} and 1 in seen
    assert is_zero(B.f29_reduce(B.limbs(0))) and is_zero(B.f29_reduce(B.limbs(B.R)))
