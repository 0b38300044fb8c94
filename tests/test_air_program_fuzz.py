"""The fuzz corpus of tests/air_program_fuzz.py on the CPU: Air::parse accepts
every raw program, the library's degree rule equals the generator's, the host
evaluator (lsp_check_constraints on a host-only context) equals the big-integer
evaluator on edge-laden traces, and the corpus keeps the coverage the device
tests (tests/test_gpu_air_program_fuzz.py) rely on."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import air_program_fuzz as F  # noqa: E402
import check_constraints_ref as ref  # noqa: E402
import preprocessed_ref as PR  # noqa: E402
from linea_stark_prover_amd.air import AirProgramConfig  # noqa: E402
from linea_stark_prover_amd.field import from_mont, to_mont  # noqa: E402

R = F.R
CORPUS = F.corpus()
H = 8


@pytest.fixture(scope="module")
def env(product_lib):
    from linea_stark_prover_amd import _lib as L
    from linea_stark_prover_amd import prover as P
    ctx = P.Context(P.StarkConfig(), device=-1)
    a, d, _ = ctx.config.seeded()
    yield dict(L=L, ctx=ctx, ad=from_mont(np.concatenate([a, d])), perm=lambda h, n: perm_rows(P, a, d, h, n))
    ctx.close()


def perm_rows(P, a, d, h, n):
    """the rows of a valid trace of the built-in permutation config of n + n columns"""
    return ref.ints(P.gen_permutation_trace(h.bit_length() - 1, n, a, d))


def _perm_of(env, case, h):
    n = [p[1] for p in case.parts if isinstance(p, tuple)]
    return env["perm"](h, n[0]) if n else None


def _desc(air):
    d = air.descriptor()
    return (ctypes.c_int32 * len(d))(*d), len(d)


def _check(env, case, rows, pubi, prows):
    pre = F.to_matrix(prows) if prows is not None else None
    got = env["ctx"].check_constraints(F.to_matrix(rows), case.air, to_mont(pubi), max_violations=64, preprocessed=pre)
    return ref.as_dict(got)


def test_corpus_shape():
    fam = [c.family for c in CORPUS if len(c.parts) == 1]
    assert (fam.count("free"), fam.count("identity"), fam.count("solvable")) == (60, 30, 20)
    assert sum(len(c.parts) > 1 for c in CORPUS) == 4
    nops = [len(p.ops) for c in CORPUS for p in c.programs]
    assert min(nops) == 1 and 150 <= max(nops) <= 260
    assert {c.prep_width for c in CORPUS} == {0, 1, 3}
    # the same seeds give the same programs
    again = F._corpus()
    assert [c.air.descriptor() for c in again] == [c.air.descriptor() for c in CORPUS]
    # every value the generator draws is canonical
    assert all(0 <= v < R for c in CORPUS for p in c.programs for v in p.consts)
    assert all(0 <= v < R for c in CORPUS for v in c.extra)
    assert all(0 <= v < R for v in F.EDGES) and len(set(F.EDGES)) == len(F.EDGES)


def test_parser_accepts_and_counts(env):
    L = env["L"]
    for c in CORPUS:
        desc, n = _desc(c.air)
        nc = ctypes.c_uint32()
        L.check(L.lib().lsp_air_num_constraints(desc, n, ctypes.byref(nc)))
        assert nc.value == sum(x.nassert for x in F.lower(c.air).configs), c
        for p in c.programs:
            assert isinstance(p, AirProgramConfig) and 1 <= len(p.ops)


def test_degrees_equal_the_tracked_ones(env):
    L = env["L"]
    for c in CORPUS:
        desc, n = _desc(c.air)
        exp = c.degrees()
        # the generator's bookkeeping is the rule of preprocessed_ref.program_degrees
        assert exp == [d for cfg in F.lower(c.air).configs for d in PR.program_degrees(cfg, F.PD)], c
        assert max(exp) <= F.MAX_DEG
        out = ctypes.c_uint32()
        for j, d in enumerate(exp):
            L.check(L.lib().lsp_air_constraint_degree(desc, n, F.PD, j, ctypes.byref(out)))
            assert out.value == d, (c, j)
        L.check(L.lib().lsp_log_quotient_degree(desc, n, F.PD, ctypes.byref(out)))
        assert out.value == c.log_q() <= env["ctx"].config.log_blowup, c


def test_host_check_equals_the_evaluator(env):
    pubs = env["ad"]
    for c in CORPUS:
        pubi = pubs + c.extra
        rows, prows = c.rows(H, pubi), c.prows(H)
        exp = F.report(c.air, rows, pubi, 64, prows)
        assert _check(env, c, rows, pubi, prows) == exp, c
        if c.family == "identity":
            assert exp["ok"], c
        elif c.family == "free" and len(c.parts) == 1 and len(c.programs[0].ops) > 3:
            assert not exp["ok"], c


def test_identity_programs_hold_on_every_trace(env):
    pubs = env["ad"]
    for c in CORPUS:
        if c.family != "identity":
            continue
        for salt in (1, 2, 3):
            pubi = pubs + [F.draw_value(random.Random(salt * 31 + c.seed)) for _ in range(2)]
            rows, prows = c.rows(H, pubi, salt=salt), c.prows(H, salt)
            got = _check(env, c, rows, pubi, prows)
            assert got["ok"] and got["failed_rows"] == 0 and got == F.report(c.air, rows, pubi, 64, prows), (c, salt)


def test_solvable_programs_hold_on_their_trace_and_break_with_it(env):
    pubs = env["ad"]
    for c in CORPUS:
        if c.family != "solvable":
            continue
        pubi = pubs + c.extra
        rows, prows = c.rows(H, pubi, _perm_of(env, c, H)), c.prows(H)
        got = _check(env, c, rows, pubi, prows)
        assert got["ok"] and got == F.report(c.air, rows, pubi, 64, prows), c
        # one defined cell bumped: the last column is program-defined in every solvable case
        rng = random.Random(c.seed)
        r_, col = rng.randrange(H), c.width - 1 - rng.randrange(c.programs[-1].nassert)
        rows[r_][col] = (rows[r_][col] + 1) % R
        exp = F.report(c.air, rows, pubi, 64, prows)
        assert _check(env, c, rows, pubi, prows) == exp, c
        # (a bumped cell goes unnoticed only where its assert's selector is off in that row)
        assert not exp["ok"] or any(F.kind(x) in (F.FIRST, F.LAST, F.TRANS) for o in c.programs[-1].ops
                                    for x in o[2:]), c


# ------------------------------------------------------- coverage conditions
def test_coverage_conditions():
    """conditions of the corpus, asserted so that an edit of the generator
    cannot silently thin what the device tests run"""
    cls = [set().union(*(F.classes(p) for p in c.programs)) for c in CORPUS]
    for form in F.FORMS:
        n = sum(form in s for s in cls)
        assert n >= 3, (form, n)
    # a regime is the launch's: the largest nslots of the descriptor
    regs = [F.regime(c.nslots) for c in CORPUS]
    for reg in F.REGIMES:
        assert regs.count(reg) >= 5, (reg, regs.count(reg))
    every = set().union(*cls)
    for k in range(10):
        assert f"assert_kind_{k}" in every and f"mul_kind_{k}" in every, k
    draws = sum(p.fuzz["draws"] for c in CORPUS for p in c.programs)
    redraws = sum(p.fuzz["redraws"] for c in CORPUS for p in c.programs)
    print(f"degree redraws: {redraws} of {draws} draws ({100.0 * redraws / draws:.1f} %)")
    assert draws > 1000 and 2 * redraws <= draws, (redraws, draws)
    # the subset of the larger heights spans the regimes and the families
    sub = F.large_subset()
    assert 10 <= len(sub) <= 14 and {F.regime(c.nslots) for c in sub} == set(F.REGIMES)
    assert {c.family for c in sub} == {"free", "identity", "solvable"} and any(len(c.parts) > 1 for c in sub)


def test_classes_names_the_forms():
    """classes() on hand-written op lists: one program per form"""
    A, S, M, Z = F.ADD, F.SUB, F.MUL, F.ASSERT
    loc, nxt, pub, cst, fst, lst, trn = (k << 24 for k in range(1, 8))

    def cl(ops, nslots=2, consts=(0, 5)):
        return F.classes(AirProgramConfig(2, nslots, list(consts), ops))

    assert "dst_is_operand" in cl([(A, 0, loc, loc), (A, 0, 0, nxt), (Z, 0, 0, 0)])
    assert "dst_is_both_operands" in cl([(A, 0, loc, nxt), (M, 0, 0, 0), (Z, 0, 0, 0)])
    assert "same_slot_twice" in cl([(A, 0, loc, nxt), (M, 1, 0, 0), (Z, 0, 1, 0)])
    assert "same_cell_twice" in cl([(M, 0, loc | 1, loc | 1), (Z, 0, 0, 0)])
    assert "const_op_const" in cl([(S, 0, cst, cst | 1), (Z, 0, 0, 0)])
    assert "selector_op_selector" in cl([(M, 0, fst, trn), (Z, 0, 0, 0)])
    assert {"assert_raw_mul", "assert_kind_0"} <= cl([(M, 0, loc, nxt), (Z, 0, 0, 0)])
    assert "assert_raw_mul" not in cl([(M, 0, loc, nxt), (A, 0, 0, loc), (Z, 0, 0, 0)])
    for name, x in (("assert_local", loc), ("assert_next", nxt), ("assert_public", pub), ("assert_const_zero", cst),
                    ("assert_const_nonzero", cst | 1), ("assert_first", fst), ("assert_last", lst),
                    ("assert_trans", trn)):
        assert {name, "nslots_0"} <= cl([(Z, 0, x, 0)], nslots=0)
    assert "overwritten_then_read" in cl([(A, 0, loc, loc), (A, 0, nxt, nxt), (Z, 0, 0, 0)]) - \
        cl([(A, 0, loc, loc), (Z, 0, 0, 0)])
    assert "sub_raw_product" in cl([(M, 0, loc, nxt), (S, 1, loc, 0), (Z, 0, 1, 0)])
    assert "sub_selector" in cl([(S, 0, loc, lst), (Z, 0, 0, 0)])
    assert {"mul_raw_raw", "mul_kind_0", "mul_kind_1"} <= cl([(M, 0, loc, nxt), (M, 1, loc, loc), (M, 0, 0, 1),
                                                                 (Z, 0, 0, 0)])
    nine = [(M, 0, loc, loc), (M, 0, 0, 0), (M, 0, 0, 0), (M, 0, 0, loc), (Z, 0, 0, 0)]
    assert "degree_9" in cl(nine) and "degree_9" not in cl(nine[:3] + nine[4:])
    chain = [(M, 0, loc, nxt)] + [(A, 0, 0, loc)] * 8 + [(Z, 0, 0, 0)]
    assert "addsub_chain_8" in cl(chain) and "addsub_chain_8" not in cl(chain[:8] + chain[9:])
    assert [F.regime(n) for n in (0, 1, 5, 6, 8, 9, 16)] == ["nslots_0", "nslots_1_5", "nslots_1_5", "nslots_6_8",
                                                              "nslots_6_8", "nslots_9_16", "nslots_9_16"]
