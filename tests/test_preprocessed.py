"""Preprocessed columns on the CPU (host-only context): the LSP_AIR_PROGRAM_PREP
descriptor (type 4, operand kinds 8 PREP_LOCAL / 9 PREP_NEXT) through Air::parse
and the degree rule, the Python encoder, the calls that refuse such an AIR
because they are given no preprocessed matrix, and the host path of
lsp_check_constraints_preprocessed against the big-integer evaluator of
tests/preprocessed_ref.py.  tests/test_gpu_preprocessed.py holds the kernels
and lsp_preprocess to the same references."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import check_constraints_ref as ref  # noqa: E402
import preprocessed_ref as PR  # noqa: E402
from linea_stark_prover_amd import air as AIR  # noqa: E402
from linea_stark_prover_amd.air import LineaAIR, ProgramBuilder, permutation_air  # noqa: E402
from linea_stark_prover_amd.field import MODULUS, to_mont  # noqa: E402


@pytest.fixture(scope="module")
def env(product_lib):
    from linea_stark_prover_amd import _lib as L
    from linea_stark_prover_amd import prover as P
    ctx = P.Context(P.StarkConfig(), device=-1)
    a, d, _ = ctx.config.seeded()
    alpha, delta = ref.pub_ints(np.concatenate([a, d]))
    yield dict(L=L, P=P, ctx=ctx, alpha=alpha, delta=delta)
    ctx.close()


def _desc(d):
    d = d.descriptor() if isinstance(d, LineaAIR) else list(d)
    return (ctypes.c_int32 * max(len(d), 1))(*d), len(d)


def _rc(L, d):
    desc, n = _desc(d)
    out = ctypes.c_uint32()
    return L.lib().lsp_air_num_constraints(desc, n, ctypes.byref(out))


def _prep(width=2, prep_width=2, nslots=1, consts=(), ops=((3, 0, 8 << 24, 9 << 24 | 1), (4, 0, 0, 0)), type_=4):
    """a one-config descriptor from raw fields"""
    cfg = AIR.AirProgramConfig(width, nslots, list(consts), [tuple(o) for o in ops], prep_width=1)
    d = [1] + cfg.encode()
    assert d[1] == 4 and d[3] == 1
    d[3] = prep_width
    if type_ == 3:  # the same ops in a type-3 config
        del d[3]
        d[1] = 3
    return d


# ---------------------------------------------------------------- encoder
def test_builder_without_preprocessed_columns_encodes_as_before():
    def prog(b):
        b.when_first_row().assert_eq(b.local[0], b.public[2])
        b.when_transition().assert_eq(b.next[1], b.local[0] * b.local[1] + 3)
        return b.build()
    plain, zero = prog(ProgramBuilder(2)), prog(ProgramBuilder(2, preprocessed_width=0))
    assert plain == zero and plain.prep_width == 0
    d = plain.encode()
    assert d == zero.encode() and d[0] == AIR.LSP_AIR_PROGRAM == 3
    # the layout of include/lsp.h, word for word: 3, width, nslots, nconst, nops, nassert, ...
    assert d[:6] == [3, 2, plain.nslots, len(plain.consts), len(plain.ops), 2]
    assert len(d) == 6 + 8 * len(plain.consts) + 4 * len(plain.ops)
    with pytest.raises(IndexError):
        ProgramBuilder(2).preprocessed[0]
    with pytest.raises(ValueError):
        ProgramBuilder(2, preprocessed_width=(1 << 20) + 1)


def test_type_4_round_trip():
    for name in PR.AIRS:
        wp, w, _ = PR.AIRS[name]
        a, b = PR.build_air(name, "a"), PR.build_air(name, "b")
        da, db = a.descriptor(), b.descriptor()
        assert da[1] == 3 and da[2] == wp + w
        assert db[1:4] == [4, w, wp] and len(db) == len(da) + 1  # the same ops, one more header word
        assert a.width == wp + w and b.width == w
        back = LineaAIR.from_descriptor(db)
        assert back.descriptor() == db and back.configs == b.configs and back.configs[0].prep_width == wp
        kinds = {x >> 24 for o in b.configs[0].ops for x in o[2:]}
        assert kinds & {8, 9} and not {x >> 24 for o in a.configs[0].ops for x in o[2:]} & {8, 9}
    assert PR.build_air("pressure", "b").configs[0].nslots >= 9  # the 128-thread block form
    assert {x >> 24 for o in PR.build_air("gated", "b").configs[0].ops for x in o[2:]} >= {8, 9}


# ----------------------------------------------------------------- parser
def test_parser_accepts_the_valid_bases(env):
    L = env["L"]
    assert _rc(L, _prep()) == L.LSP_OK
    assert _rc(L, _prep(prep_width=1, ops=[(4, 0, 8 << 24, 0)], nslots=0)) == L.LSP_OK
    assert _rc(L, _prep(prep_width=1 << 20, ops=[(4, 0, 9 << 24 | ((1 << 20) - 1), 0)], nslots=0)) == L.LSP_OK
    # beside main cells, and beside a built-in config
    assert _rc(L, _prep(ops=[(1, 0, 1 << 24 | 1, 8 << 24 | 1), (4, 0, 0, 0)])) == L.LSP_OK
    for name in PR.AIRS:
        assert _rc(L, PR.build_air(name, "b")) == L.LSP_OK
    mixed = LineaAIR([permutation_air(1).configs[0], PR.build_air("keyed", "b").configs[0]])
    assert _rc(L, mixed) == L.LSP_OK


MALFORMED = {
    "column = prep_width": _prep(ops=[(3, 0, 8 << 24 | 2, 9 << 24), (4, 0, 0, 0)]),
    "next column = prep_width": _prep(ops=[(3, 0, 8 << 24, 9 << 24 | 2), (4, 0, 0, 0)]),
    "asserted column = prep_width": _prep(prep_width=1, nslots=0, ops=[(4, 0, 8 << 24 | 1, 0)]),
    "prep_width zero": _prep(prep_width=0),
    "prep_width negative": _prep(prep_width=-1),
    "prep_width past 2^20": _prep(prep_width=(1 << 20) + 1),
    "kind 8 inside type 3": _prep(type_=3, ops=[(3, 0, 8 << 24, 1 << 24), (4, 0, 0, 0)]),
    "kind 9 inside type 3": _prep(type_=3, ops=[(4, 0, 9 << 24, 0)], nslots=0),
    "kind 10 inside type 4": _prep(ops=[(4, 0, 10 << 24, 0)], nslots=0),
    "truncated by one word": _prep()[:-1],
    "truncated after the type": _prep()[:2],
    "truncated after prep_width": _prep()[:4],
    "truncated in the header": _prep()[:6],
    "truncated in the constants": _prep(consts=[1, 2], ops=[(4, 0, 4 << 24, 0)], nslots=0)[:14],
    "trailing word": _prep() + [0],
    # the header of a type-3 config under a type-4 type word (and the other way round)
    "type 3 header as type 4": [1, 4] + _prep(type_=3, ops=[(4, 0, 1 << 24, 0)], nslots=0)[2:],
    "type 4 header as type 3": [1, 3] + _prep()[2:],
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_parser_rejects(env, case):
    L = env["L"]
    assert _rc(L, MALFORMED[case]) == L.LSP_E_ARG
    msg = L.lib().lsp_last_error(None).decode()
    if "column =" in case or "kind" in case:
        assert " op " in msg, msg  # the message names the op


def test_every_truncation_is_rejected(env):
    L = env["L"]
    d = PR.build_air("gated", "b").descriptor()
    assert _rc(L, d) == L.LSP_OK
    for n in range(len(d)):
        assert _rc(L, d[:n]) == L.LSP_E_ARG, n


def _degrees(L, air, pd):
    desc, n = _desc(air)
    nc, out, got = ctypes.c_uint32(), ctypes.c_uint32(), []
    L.check(L.lib().lsp_air_num_constraints(desc, n, ctypes.byref(nc)))
    for j in range(nc.value):
        L.check(L.lib().lsp_air_constraint_degree(desc, n, pd, j, ctypes.byref(out)))
        got.append(out.value)
    return got


@pytest.mark.parametrize("name", sorted(PR.AIRS))
def test_a_fixed_cell_has_degree_one(env, name):
    L = env["L"]
    a, b = PR.build_air(name, "a"), PR.build_air(name, "b")
    for pd in (0, 1, 2):
        exp = PR.program_degrees(b.configs[0], pd)
        assert _degrees(L, b, pd) == exp == _degrees(L, a, pd)
    lq = ctypes.c_uint32()
    desc, n = _desc(b)
    L.check(L.lib().lsp_log_quotient_degree(desc, n, 1, ctypes.byref(lq)))
    assert lq.value == PR.LOG_Q[name] and max(PR.program_degrees(b.configs[0], 1)) == {0: 2, 2: 4}[lq.value]
    # a product of two fixed cells alone has degree 2
    assert _degrees(L, _prep(), 1) == [2]


def test_constraint_info_reports_the_type(env):
    L = env["L"]
    air = LineaAIR([permutation_air(1).configs[0], PR.build_air("keyed", "b").configs[0]])
    desc, n = _desc(air)
    cfg, typ, kind, tab = ctypes.c_uint32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    L.check(L.lib().lsp_air_constraint_info(desc, n, 5, ctypes.byref(cfg), ctypes.byref(typ), ctypes.byref(kind),
                                            ctypes.byref(tab)))
    assert (cfg.value, typ.value, kind.value, tab.value) == (1, L.LSP_AIR_PROGRAM_PREP, L.LSP_CONSTRAINT_PROGRAM, -1)
    assert len(air.constraint_names()) == 6 and air.constraint_names()[5] == "cfg 1 program: x' = x^2 + k"


# ---------------------------------------------------------------- refusals
def _case(env, name, h):
    fixed, main, extra = PR.build_rows(name, h)
    pubi = [env["alpha"], env["delta"]] + extra
    return fixed, main, pubi


def test_calls_without_a_preprocessed_matrix_refuse(env):
    L, ctx = env["L"], env["ctx"]
    air = PR.build_air("keyed", "b")
    fixed, main, pubi = _case(env, "keyed", 8)
    pub = np.ascontiguousarray(to_mont(pubi))
    trace = np.ascontiguousarray(PR.to_matrix(main))
    desc, n = _desc(air)
    proof = b"LSPPRF02" + bytes(256)
    assert L.lib().lsp_verify(ctx.h, desc, n, pub.ctypes.data, 3, proof, len(proof)) == L.LSP_E_ARG
    assert "preprocessed" in L.lib().lsp_last_error(None).decode()
    s = L.LspCheckSummary()
    rc = L.lib().lsp_check_constraints(ctx.h, trace.ctypes.data, 8, 1, desc, n, pub.ctypes.data, 3, 0,
                                       ctypes.byref(s), None, None, None, 0, None)
    assert rc == L.LSP_E_ARG and "the AIR reads preprocessed columns" in L.lib().lsp_last_error(ctx.h).decode()
    with pytest.raises(L.LspError) as e:
        ctx.check_constraints(trace, air, pub)
    assert e.value.code == L.LSP_E_ARG
    with pytest.raises(L.LspError) as e:
        ctx.verify(proof, air, pub)
    assert e.value.code == L.LSP_E_ARG
    # the same verdict with a matrix that is too narrow, and with none under the new entry point
    air2 = PR.build_air("gated", "b")
    f2, m2, p2 = _case(env, "gated", 8)
    with pytest.raises(L.LspError) as e:
        ctx.check_constraints(PR.to_matrix(m2), air2, to_mont(p2), preprocessed=PR.to_matrix(f2)[:, :1])
    assert e.value.code == L.LSP_E_ARG and "preprocessed columns" in str(e.value)
    desc2, n2 = _desc(air2)
    rc = L.lib().lsp_check_constraints_preprocessed(ctx.h, trace.ctypes.data, 8, 1, None, 0, desc2, n2,
                                                    pub.ctypes.data, 3, 0, ctypes.byref(s), None, None, None, 0, None)
    assert rc == L.LSP_E_ARG
    # an AIR that reads none is served by the new entry point too (the matrix is ignored)
    fib = ProgramBuilder(1)
    fib.when_first_row().assert_eq(fib.local[0], fib.public[2])
    assert ctx.check_constraints(trace, LineaAIR([fib.build()]), pub, preprocessed=PR.to_matrix(fixed)).ok


# -------------------------------------------------------------- host check
def _cells(name, h):
    """(where, row, column) of the planted faults: main and fixed cells, first / inner / last rows"""
    wp, w, _ = PR.AIRS[name]
    rows = sorted({0, h // 2, h - 1})
    return [("main", r, w - 1) for r in rows] + [("fixed", r, wp - 1) for r in rows]


@pytest.mark.parametrize("h", [2, 8])
@pytest.mark.parametrize("name", sorted(PR.AIRS))
def test_host_check_equals_the_evaluator(env, name, h):
    ctx = env["ctx"]
    air_a, air_b = PR.build_air(name, "a"), PR.build_air(name, "b")
    fixed, main, pubi = _case(env, name, h)
    pub = to_mont(pubi)
    exp = PR.report(air_b, main, pubi, 16, fixed)
    assert exp["ok"] and exp == PR.report(air_a, PR.joined(fixed, main), pubi, 16)
    got = ctx.check_constraints(PR.to_matrix(main), air_b, pub, preprocessed=PR.to_matrix(fixed))
    assert ref.as_dict(got) == exp
    seen_bad = 0
    for where, r_, c in _cells(name, h):
        ff, mm = [list(x) for x in fixed], [list(x) for x in main]
        (mm if where == "main" else ff)[r_][c] = ((mm if where == "main" else ff)[r_][c] + 1) % MODULUS
        exp = PR.report(air_b, mm, pubi, 16, ff)
        # layout a is the same AIR: the existing entry point gives the same report
        assert exp == PR.report(air_a, PR.joined(ff, mm), pubi, 16)
        got = ctx.check_constraints(PR.to_matrix(mm), air_b, pub, preprocessed=PR.to_matrix(ff))
        assert ref.as_dict(got) == exp
        assert ref.as_dict(ctx.check_constraints(PR.to_matrix(PR.joined(ff, mm)), air_a, pub)) == exp
        if not exp["ok"]:
            seen_bad += 1
            assert str(got).startswith(f"constraints had nonzero value on row {exp['first'][0]}: "
                                       f"constraint {exp['first'][1]} ")
    assert seen_bad >= 3  # main and fixed faults both show
    # a changed public value breaks the constraint that reads it
    pubi[-1] = (pubi[-1] + 1) % MODULUS
    exp = PR.report(air_b, main, pubi, 16, fixed)
    assert not exp["ok"]
    got = ctx.check_constraints(PR.to_matrix(main), air_b, to_mont(pubi), preprocessed=PR.to_matrix(fixed))
    assert ref.as_dict(got) == exp


def test_mixed_with_a_built_in_config(env):
    """a built-in permutation config beside a type-4 program: the program's
    main column follows the permutation's, its fixed column is the matrix's"""
    P, ctx = env["P"], env["ctx"]
    a, d, _ = ctx.config.seeded()
    tp = ref.ints(P.gen_permutation_trace(3, 1, a, d))  # 8 rows x 4 columns
    fixed, main, pubi = _case(env, "keyed", 8)
    prog = PR.build_air("keyed", "b").configs[0]
    prog.shift(4)
    air = LineaAIR([permutation_air(1).configs[0], prog])
    assert air.descriptor()[-len(prog.encode()):][:3] == [4, 5, 1]  # shift moves main columns only
    rows = [list(x) + list(y) for x, y in zip(tp, main)]
    pub = to_mont(pubi)
    rep = ctx.check_constraints(PR.to_matrix(rows), air, pub, preprocessed=PR.to_matrix(fixed))
    assert rep.ok and len(rep.counts) == 6
    fixed[3][0] = (fixed[3][0] + 1) % MODULUS
    rep = ctx.check_constraints(PR.to_matrix(rows), air, pub, preprocessed=PR.to_matrix(fixed))
    assert rep.first == (3, 5) and rep.failed_rows == 1 and rep.counts == [0, 0, 0, 0, 0, 1]
