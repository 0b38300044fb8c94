"""LSP_AIR_PROGRAM on the CPU: the Python encoder, Air::parse's limits, the
degree rule, the host evaluator (lsp_check_constraints on a host-only context,
lsp_verify) and the integer model of the check kernel's zero test.  The built-in
configs restated as programs must behave exactly as the built-in descriptor
does; AIRs the oracle does not know are held to the big-integer evaluator of
tests/air_program_ref.py.  tests/test_gpu_air_program.py holds the kernels to
the same references."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import air_program_ref as A  # noqa: E402
import check_constraints_ref as ref  # noqa: E402
from linea_stark_prover_amd import air as AIR  # noqa: E402
from linea_stark_prover_amd.air import LineaAIR, ProgramBuilder, lower, permutation_air  # noqa: E402
from linea_stark_prover_amd.field import MODULUS, to_mont  # noqa: E402


@pytest.fixture(scope="module")
def env(product_lib):
    from linea_stark_prover_amd import _lib as L
    from linea_stark_prover_amd import prover as P
    ctx = P.Context(P.StarkConfig(), device=-1)
    a, d, _ = ctx.config.seeded()
    pub = np.concatenate([a, d])
    alpha, delta = ref.pub_ints(pub)
    yield dict(L=L, P=P, ctx=ctx, pub=pub, alpha=alpha, delta=delta, a=a, d=d)
    ctx.close()


def _desc(d):
    d = d.descriptor() if isinstance(d, LineaAIR) else list(d)
    return (ctypes.c_int32 * max(len(d), 1))(*d), len(d)


def _log_q(L, air, pd):
    desc, n = _desc(air)
    out = ctypes.c_uint32()
    L.check(L.lib().lsp_log_quotient_degree(desc, n, pd, ctypes.byref(out)))
    return out.value


def _degrees(L, air, pd):
    desc, n = _desc(air)
    nc, out, got = ctypes.c_uint32(), ctypes.c_uint32(), []
    L.check(L.lib().lsp_air_num_constraints(desc, n, ctypes.byref(nc)))
    for j in range(nc.value):
        L.check(L.lib().lsp_air_constraint_degree(desc, n, pd, j, ctypes.byref(out)))
        got.append(out.value)
    assert L.lib().lsp_air_constraint_degree(desc, n, pd, nc.value, ctypes.byref(out)) == L.LSP_E_ARG
    return got


# ---------------------------------------------------------------- encoder
def test_round_trip():
    for air in (lower(permutation_air(3)), A.fibonacci_air(), A.sbox_air(9), A.pressure_air(16),
                LineaAIR([permutation_air(2).configs[0], A.fibonacci_air().configs[0]])):
        d = air.descriptor()
        back = LineaAIR.from_descriptor(d)
        assert back.descriptor() == d and back.configs == air.configs
        assert len(back.constraint_names()) == len(air.constraint_names())
    air = A.fibonacci_air()
    assert air.constraint_names()[3] == "cfg 0 program: b' = a + b"
    assert LineaAIR.from_descriptor(air.descriptor()).constraint_names()[3] == "cfg 0 program: assert[3]"
    assert air.width == 2 and lower(permutation_air(3)).width == 8


def test_shift_moves_columns_only():
    cfg = A.fibonacci_air().configs[0]
    before = list(cfg.ops)
    cfg.shift(5)
    assert cfg.desc_width == 7 and cfg.width() == 2
    for (c0, d0, a0, b0), (c1, d1, a1, b1) in zip(before, cfg.ops):
        assert (c0, d0) == (c1, d1)
        for x, y in ((a0, a1), (b0, b1)):
            assert y == (x + 5 if x >> 24 in (1, 2) and (c0 != 4 or x is a0) else x)


def test_cse_merges_a_repeated_subexpression():
    b = ProgramBuilder(2)
    e = b.local[0] * b.next[1] + 3
    b.assert_zero(e * e - (b.local[0] * b.next[1] + 3))
    cfg = b.build()
    muls = [o for o in cfg.ops if o[0] == AIR.OP_MUL]
    assert len(muls) == 2 and len(cfg.ops) == 5  # x y, + 3, e e, -, assert
    # integer constants fold, also across a negation
    b = ProgramBuilder(1)
    b.assert_zero(b.local[0] - (b.const(2) * 3 - 7))
    cfg = b.build()
    assert cfg.consts == [MODULUS - 1] and len(cfg.ops) == 2
    rows = [[MODULUS - 1]] * 2
    assert A.report(LineaAIR([cfg]), rows, [0, 0], 1)["ok"]


def test_forty_live_values_raise():
    b = ProgramBuilder(40)
    t = [b.local[i] * b.next[i] for i in range(40)]
    s, u = t[0], t[39]
    for x in t[1:]:
        s = s + x
    for x in reversed(t[:39]):
        u = u * x
    b.assert_zero(s)
    b.assert_zero(u)
    with pytest.raises(ValueError, match="more than 16 slots"):
        b.build()
    assert A.pressure_air(16).configs[0].nslots == 16 and A.pressure_air(8).configs[0].nslots == 8


def test_horner_chain_needs_few_slots():
    b = ProgramBuilder(4096)
    acc = b.const(0)
    for i in range(4096):
        acc = acc * b.public[0] + b.local[i]
    b.assert_zero(acc - b.public[1])
    cfg = b.build()
    assert cfg.nslots <= 3 and len(cfg.ops) == 2 * 4096 + 2
    # the deeper side first: a right-leaning sum of products needs 2 slots, not one per term
    b = ProgramBuilder(64)
    e = b.local[63] * b.next[63]
    for i in range(62, -1, -1):
        e = b.local[i] * b.next[i] + e
    b.assert_zero(e)
    assert b.build().nslots == 2


def test_builder_rejects_what_the_format_cannot_hold():
    b = ProgramBuilder(2)
    with pytest.raises(IndexError):
        b.local[2]
    with pytest.raises(ValueError):
        b.build()  # no assert
    with pytest.raises(ValueError):
        ProgramBuilder(1).assert_zero(b.local[0])  # another builder's expression
    with pytest.raises(TypeError):
        b.local[0] + 1.5


# ----------------------------------------------------------------- parser
def _rc(L, d):
    desc, n = _desc(d)
    out = ctypes.c_uint32()
    return L.lib().lsp_air_num_constraints(desc, n, ctypes.byref(out))


def _prog(width=2, nslots=1, consts=(), ops=((3, 0, 1 << 24, 2 << 24), (4, 0, 0, 0)), nassert=None):
    """a one-config descriptor from raw fields"""
    cfg = AIR.AirProgramConfig(width, nslots, list(consts), [tuple(o) for o in ops])
    d = [1] + cfg.encode()
    if nassert is not None:
        d[6] = nassert
    return d


def test_parser_accepts_the_valid_base(env):
    assert _rc(env["L"], _prog()) == env["L"].LSP_OK
    assert _rc(env["L"], _prog(nslots=0, ops=[(4, 0, 1 << 24 | 1, 0)])) == env["L"].LSP_OK
    assert _rc(env["L"], _prog(consts=[MODULUS - 1], ops=[(4, 0, 4 << 24, 0)])) == env["L"].LSP_OK
    assert _rc(env["L"], _prog(nslots=16, ops=[(1, 15, 5 << 24, 7 << 24), (4, 0, 15, 0)])) == env["L"].LSP_OK


MALFORMED = {
    "17 slots": _prog(nslots=17),
    "negative slots": _prog(nslots=-1),
    "no ops": _prog(ops=[]),
    "no assert": _prog(ops=[(3, 0, 1 << 24, 2 << 24)]),
    "nassert too small": _prog(ops=[(4, 0, 1 << 24, 0), (4, 0, 2 << 24, 0)], nassert=1),
    "nassert too large": _prog(nassert=2),
    "nassert zero": _prog(nassert=0),
    "width zero": _prog(width=0, nslots=0, ops=[(4, 0, 5 << 24, 0)]),
    "width past 2^20": _prog(width=(1 << 20) + 1),
    "column = width": _prog(ops=[(3, 0, 1 << 24 | 2, 2 << 24), (4, 0, 0, 0)]),
    "next column = width": _prog(ops=[(3, 0, 1 << 24, 2 << 24 | 2), (4, 0, 0, 0)]),
    "constant = r": _prog(consts=[MODULUS], ops=[(4, 0, 4 << 24, 0)]),
    "constant 2^256 - 1": _prog(consts=[(1 << 256) - 1], ops=[(4, 0, 4 << 24, 0)]),
    "constant index past nconst": _prog(consts=[1], ops=[(4, 0, 4 << 24 | 1, 0)]),
    "slot read before written": _prog(ops=[(4, 0, 0, 0)]),
    "slot read in its own first write": _prog(ops=[(1, 0, 0, 1 << 24), (4, 0, 0, 0)]),
    "slot past nslots": _prog(ops=[(3, 0, 1 << 24, 2 << 24), (4, 0, 1, 0)]),
    "destination past nslots": _prog(ops=[(3, 1, 1 << 24, 2 << 24), (4, 0, 1 << 24, 0)]),
    "negative destination": _prog(ops=[(3, -1, 1 << 24, 2 << 24), (4, 0, 1 << 24, 0)]),
    "opcode 0": _prog(ops=[(0, 0, 1 << 24, 2 << 24), (4, 0, 1 << 24, 0)]),
    "opcode 5": _prog(ops=[(5, 0, 1 << 24, 2 << 24), (4, 0, 1 << 24, 0)]),
    "operand kind 8": _prog(ops=[(4, 0, 8 << 24, 0)]),
    "operand kind 255": _prog(ops=[(4, 0, -1, 0)]),
    "assert with a destination": _prog(ops=[(4, 1, 1 << 24, 0)]),
    "assert with a second operand": _prog(ops=[(4, 0, 1 << 24, 1 << 24)]),
    "selector with a payload": _prog(ops=[(4, 0, 5 << 24 | 1, 0)]),
    "public index 2^16": _prog(ops=[(4, 0, 3 << 24 | 1 << 16, 0)]),
    "truncated": _prog()[:-1],
    "truncated in the constants": _prog(consts=[1, 2], ops=[(4, 0, 4 << 24, 0)])[:12],
    "trailing word": _prog() + [0],
    "nconst negative": [1, 3, 2, 1, -1, 1, 1, 4, 0, 1 << 24, 0],
    "nconst past 2^16": [1, 3, 2, 1, (1 << 16) + 1, 1, 1],
    "nops past 2^20": [1, 3, 2, 1, 0, (1 << 20) + 1, 1],
    "unknown config type": [1, 4, 2, 1, 0, 1, 1, 4, 0, 1 << 24, 0],
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_parser_rejects(env, case):
    L = env["L"]
    assert _rc(L, MALFORMED[case]) == L.LSP_E_ARG
    msg = L.lib().lsp_last_error(None).decode()
    if any(w in case for w in ("slot read", "past nslots", "opcode", "operand kind", "assert with", "selector",
                               "column =", "public index", "constant index", "destination")):
        assert " op " in msg, msg  # the message names the op


def test_checked_at_the_call(env):
    """a column >= w and a PUBLIC k >= npub are errors where w and npub are known"""
    L, ctx = env["L"], env["ctx"]
    air = A.fibonacci_air()
    rows, extra = A.fibonacci_rows(8)
    trace = A.rows_to_trace(rows)
    pub4 = to_mont([env["alpha"], env["delta"]] + extra)
    assert ctx.check_constraints(trace, air, pub4).ok
    for bad_pub in (pub4[:3], pub4[:2]):
        with pytest.raises(L.LspError) as e:
            ctx.check_constraints(trace, air, bad_pub)
        assert e.value.code == L.LSP_E_ARG and "public value" in str(e.value)
    with pytest.raises(L.LspError) as e:
        ctx.check_constraints(trace[:, :1], air, pub4)
    assert e.value.code == L.LSP_E_ARG
    # the verifier: a proof is only parsed once the public values fit
    assert not ctx.verify(b"LSPPRF02" + bytes(64), air, pub4)
    assert not ctx.verify(b"LSPPRF02" + bytes(64), air, pub4[:3])


def test_seeded_mutations_never_crash(env):
    """single-word mutations of valid descriptors through four entry points: an
    error is LSP_E_ARG (lsp_verify: or a rejected proof), a mutation that stays
    well-formed may be accepted, and all four agree on which it is"""
    L, ctx = env["L"], env["ctx"]
    rows, extra = A.fibonacci_rows(8)
    trace = np.ascontiguousarray(A.rows_to_trace(rows))
    pub = np.ascontiguousarray(to_mont([env["alpha"], env["delta"]] + extra))
    proof = b"LSPPRF02" + bytes(256)
    mixed = LineaAIR([A.fibonacci_air().configs[0], permutation_air(1).configs[0]])
    mixed.configs[1].shift(2)  # columns 2..5: past the trace's width, so only the parser's verdict is compared
    rng = random.Random(2024)
    picks = [0, 1, -1, 2, 3, 4, 5, 16, 17, 1 << 16, 1 << 20, 1 << 24, 3 << 24, 4 << 24 | 5, 8 << 24, -(1 << 31),
             (1 << 31) - 1]
    accepted = rejected = 0
    for base in (A.fibonacci_air().descriptor(), A.sbox_air(5).descriptor(), mixed.descriptor()):
        for _ in range(150):
            d = list(base)
            k = rng.randrange(len(d))
            v = rng.choice(picks) if rng.random() < 0.7 else rng.randrange(-(1 << 31), 1 << 31)
            if rng.random() < 0.2:
                v = d[k] ^ (1 << rng.randrange(32))
                v = v - (1 << 32) if v >> 31 else v
            d[k] = v
            desc, n = _desc(d)
            out = ctypes.c_uint32()
            r0 = L.lib().lsp_air_num_constraints(desc, n, ctypes.byref(out))
            r1 = L.lib().lsp_log_quotient_degree(desc, n, 1, ctypes.byref(out))
            assert r0 == r1 and r0 in (L.LSP_OK, L.LSP_E_ARG)
            r2 = L.lib().lsp_verify(ctx.h, desc, n, pub.ctypes.data, 4, proof, len(proof))
            assert r2 == (L.LSP_E_VERIFY if r0 == L.LSP_OK else L.LSP_E_ARG)
            s = L.LspCheckSummary()
            r3 = L.lib().lsp_check_constraints(ctx.h, trace.ctypes.data, 8, 2, desc, n, pub.ctypes.data, 4, 0,
                                               ctypes.byref(s), None, None, None, 0, None)
            assert r3 in (L.LSP_OK, L.LSP_E_ARG) and (r3 == L.LSP_E_ARG or r0 == L.LSP_OK)
            accepted += r0 == L.LSP_OK
            rejected += r0 != L.LSP_OK
    assert accepted > 20 and rejected > 100


# ----------------------------------------------------------------- degree
def _lookup_airs(env):
    P = env["P"]
    return [P.gen_wide_trace(1, env["a"], env["d"], **ref.MIXED)[1], P.gen_wide_trace(1, env["a"], env["d"])[1]]


def test_lowered_degrees_equal_the_built_in(env):
    L = env["L"]
    for air in [permutation_air(n) for n in (1, 3, 6, 12)] + _lookup_airs(env):
        low = lower(air)
        assert low.width == air.width
        for pd in (0, 1):
            assert _log_q(L, low, pd) == _log_q(L, air, pd)
            got = _degrees(L, low, pd)
            assert got == [x for c in low.configs for x in A.program_degrees(c, pd)]
            assert got == _degrees(L, air, pd)  # the built-in's, constraint by constraint
            assert max(got) - 1 <= 1 << _log_q(L, air, pd)
    # the ZERO start of the Horner sums shows at public_degree 2: the lowering keeps it
    assert _degrees(L, lower(permutation_air(1)), 2) == _degrees(L, permutation_air(1), 2)


def test_new_air_degrees(env):
    L = env["L"]
    assert _degrees(L, A.fibonacci_air(), 1) == [2, 2, 1, 1, 2] and _log_q(L, A.fibonacci_air(), 1) == 0
    assert _degrees(L, A.sbox_air(5), 1) == [2, 5] and _log_q(L, A.sbox_air(5), 1) == 2
    assert _degrees(L, A.sbox_air(9), 1) == [2, 9] and _log_q(L, A.sbox_air(9), 1) == 3
    # a degree-10 assert needs 16 quotient chunks: past the default blowup of 8, and
    # lsp_air_constraint_degree names the constraint (the prove call's answer
    # is in tests/test_gpu_air_program.py: it needs a device)
    air = A.sbox_air(10)
    assert _log_q(L, air, 1) == 4 > env["ctx"].config.log_blowup
    d = _degrees(L, air, 1)
    assert d.index(max(d)) == 1 and max(d) == 10
    assert env["ctx"].constraint_degrees(air) == d and air.constraint_names()[1] == "cfg 0 program: x' = x^10 + c"
    desc, n = _desc(air)
    assert L.lib().lsp_air_constraint_degree(desc, n, -1, 0, ctypes.byref(ctypes.c_uint32())) == L.LSP_E_ARG
    assert L.lib().lsp_air_constraint_degree(desc, n, 1, 0, None) == L.LSP_E_ARG
    assert L.lib().lsp_air_constraint_degree(None, 0, 1, 0, ctypes.byref(ctypes.c_uint32())) == L.LSP_E_ARG


def test_constraint_info_reports_programs(env):
    L = env["L"]
    air = LineaAIR([permutation_air(1).configs[0], A.fibonacci_air().configs[0]])
    desc, n = _desc(air)
    names = air.constraint_names()
    assert len(names) == 9
    for j in range(9):
        cfg, typ, kind, tab = ctypes.c_uint32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        L.check(L.lib().lsp_air_constraint_info(desc, n, j, ctypes.byref(cfg), ctypes.byref(typ),
                                                ctypes.byref(kind), ctypes.byref(tab)))
        if j < 4:
            assert (cfg.value, typ.value) == (0, L.LSP_AIR_PERMUTATION)
        else:
            assert (cfg.value, typ.value, kind.value, tab.value) == (1, L.LSP_AIR_PROGRAM, L.LSP_CONSTRAINT_PROGRAM, -1)
            assert names[j].startswith("cfg 1 program: ")


# ------------------------------------------------------------- host check
@pytest.fixture(scope="module")
def built_in(env):
    P = env["P"]
    tp = P.gen_permutation_trace(6, 3, env["a"], env["d"])
    tm, am = P.gen_wide_trace(6, env["a"], env["d"], **ref.MIXED)
    return {"perm": (tp, permutation_air(3), ref.ints(tp)), "mixed": (tm, am, ref.ints(tm))}


def _same_report(ctx, trace, air, low, pub, cap=64):
    a = ctx.check_constraints(trace, air, pub, max_violations=cap)
    b = ctx.check_constraints(trace, low, pub, max_violations=cap)
    assert ref.as_dict(a) == ref.as_dict(b)
    return a


@pytest.mark.parametrize("which", ["perm", "mixed"])
def test_lowered_host_check_equals_built_in(env, built_in, which):
    trace, air, rows = built_in[which]
    h = len(rows)
    low = lower(air)
    half = lower(air, which={0}) if which == "perm" else lower(air, which={1, 2})  # a mixed descriptor
    assert _same_report(env["ctx"], trace, air, low, env["pub"]).ok
    for cls, col in sorted(ref.column_classes(air).items()):
        for r_ in (0, 1, h - 2, h - 1):
            t, rr = ref.tamper(trace, rows, r_, col)
            rep = _same_report(env["ctx"], t, air, low, env["pub"])
            # and both are the oracle's
            assert ref.as_dict(rep) == ref.oracle_report(air, rr, env["alpha"], env["delta"], 64)
        _same_report(env["ctx"], t, air, half, env["pub"])
    bad = to_mont([(env["alpha"] + 1) % MODULUS, env["delta"]])
    assert not _same_report(env["ctx"], trace, air, low, bad).ok


# --------------------------------------------------------------- new AIRs
def _new_airs():
    out = []
    air = A.fibonacci_air()
    rows, extra = A.fibonacci_rows(32)
    out.append(("fibonacci", air, rows, extra, [(0, 0), (0, 1), (7, 0), (31, 1)]))
    for d in (5, 9):
        rows, extra = A.sbox_rows(32, d)
        out.append((f"sbox{d}", A.sbox_air(d), rows, extra, [(0, 0), (13, 0), (31, 0)]))
    for n in (8, 16):
        rows, extra = A.pressure_rows(32, n)
        out.append((f"slots{n}", A.pressure_air(n), rows, extra, [(5, n - 2)]))
    air, k = A.long_air()
    rows, extra = A.long_rows(32, k)
    out.append(("long", air, rows, extra, [(9, 0)]))
    return out


@pytest.mark.parametrize("name,air,rows,extra,cells", _new_airs(), ids=[x[0] for x in _new_airs()])
def test_new_airs_against_the_evaluator(env, name, air, rows, extra, cells):
    ctx = env["ctx"]
    pubi = [env["alpha"], env["delta"]] + extra
    pub = to_mont(pubi)
    exp = A.report(air, rows, pubi, 16)
    assert exp["ok"]
    assert ref.as_dict(ctx.check_constraints(A.rows_to_trace(rows), air, pub)) == exp
    for r_, c in cells:
        rr = [list(x) for x in rows]
        rr[r_][c] = (rr[r_][c] + 1) % MODULUS
        exp = A.report(air, rr, pubi, 16)
        assert not exp["ok"]
        rep = ctx.check_constraints(A.rows_to_trace(rr), air, pub)
        assert ref.as_dict(rep) == exp
        assert str(rep).startswith(f"constraints had nonzero value on row {exp['first'][0]}: "
                                   f"constraint {exp['first'][1]} ")
    # a changed public value breaks the constraint that reads it
    pubi[-1] = (pubi[-1] + 1) % MODULUS
    exp = A.report(air, rows, pubi, 16)
    assert not exp["ok"]
    assert ref.as_dict(ctx.check_constraints(A.rows_to_trace(rows), air, to_mont(pubi))) == exp


def test_slotless_program(env):
    air = A.slotless_air()
    assert air.configs[0].nslots == 0
    rows = [[i + 1, 0] for i in range(8)]
    pubi = [env["alpha"], env["delta"]]
    assert env["ctx"].check_constraints(A.rows_to_trace(rows), air, to_mont(pubi)).ok
    rows[3][1] = 9
    rep = env["ctx"].check_constraints(A.rows_to_trace(rows), air, to_mont(pubi))
    assert ref.as_dict(rep) == A.report(air, rows, pubi, 16) and rep.first == (3, 0)


# --------------------------------------------------------------- verifier
@pytest.mark.parametrize("logn,ncols", [(3, 3), (5, 6), (7, 3)])
def test_verifier_accepts_oracle_proofs_with_the_lowered_air(env, oracle_lib, logn, ncols):
    """the proofs of test_host.py::test_product_verifier_accepts_oracle_proofs"""
    ctx = env["ctx"]
    p = oracle_lib.setup()
    tb, w = oracle_lib.gen_perm_trace(p, logn, ncols)
    proof = oracle_lib.prove(p, tb, 1 << logn, w, oracle_lib.perm_air(ncols))
    pub = np.concatenate([np.array(p.alpha, np.uint64).reshape(1, 4), np.array(p.delta, np.uint64).reshape(1, 4)])
    air = lower(permutation_air(ncols))
    assert ctx.verify(proof, permutation_air(ncols), pub) and ctx.verify(proof, air, pub)
    rng = np.random.default_rng(logn)
    for off in rng.integers(28, len(proof), 6):
        bad = bytearray(proof)
        bad[int(off)] ^= 1 << int(rng.integers(0, 8))
        assert not ctx.verify(bytes(bad), air, pub)
    pub2 = pub.copy()
    pub2[1, 0] ^= np.uint64(1)
    assert not ctx.verify(proof, air, pub2)
    # another program over the same columns is another statement
    assert not ctx.verify(proof, lower(permutation_air(ncols + 1)), pub) or ncols + 1 > w


# ------------------------------------------------------- zero-test bound
def test_zero_test_bound_of_program_asserts():
    """k_check.hip passes a program's asserted operand through f29_reduce_qt
    before f29_is_zero_mod_r.  The operand may be a raw product (normalised,
    < 8.92 r for inputs < 8.92 r -- the closure k_air_prog.hpp states), a 0/1
    selector, a constant or a loaded cell: after the one reduction it is
    normalised and < 2 r, where "limbs all zero or r's" is exactly "zero mod r"."""
    import test_f29_bounds as B

    def is_zero(o):
        return all(x == 0 for x in o) or o == B.P29

    def reduced(v):
        o = B.f29_reduce_qt(v)
        B.check_reduced(o, B.val(v))
        assert is_zero(o) == (B.val(v) % B.R == 0)
        return o

    rng = random.Random(261)
    top = 892 * B.R // 100
    worst = 0
    for _ in range(1500):
        # operands anywhere below 8.92 r, in any representative of their class
        x, y = rng.randrange(top), rng.randrange(top)
        p, _w = B.f29_mul(B.limbs(x), B.limbs(y))
        assert all(v <= B.MASK for v in p[:8]) and B.val(p) < top  # closed: a product is an operand again
        worst = max(worst, B.val(p))
        reduced(p)
        # a product that is zero mod r: one factor a multiple of r
        k = rng.randrange(9)
        if k * B.R < top:
            z, _w = B.f29_mul(B.limbs(x), B.limbs(k * B.R))
            assert B.val(z) % B.R == 0 and B.val(z) < top
            assert is_zero(reduced(z))
        # sums and differences of operands, as Q29::add / sub form them, are reduced operands
        s = [a + b for a, b in zip(B.limbs(x), B.limbs(y))]
        o = reduced(s)
        assert B.val(o) < 2 * B.R
        d = [a + B.L16[i] - b for i, (a, b) in enumerate(zip(B.limbs(x), B.limbs(y)))]
        assert min(d) >= 0
        reduced(d)
        # a constant: canonical c 2^261 mod r
        c = rng.randrange(B.R)
        reduced(B.limbs(c))
    assert worst < top
    # the extremes: both factors at the bound
    p, _w = B.f29_mul(B.limbs(top - 1), B.limbs(top - 1))
    assert B.val(p) < top
    reduced(p)
    # the 0/1 selectors: 0 is all-zero limbs; 1 is f29_from_fr(one) = f29_reduce((2^256 mod r) << 5)
    one = B.f29_reduce(B.limbs((pow(2, 256, B.R)) << 5))
    assert B.val(one) < 2 * B.R and B.val(one) % B.R == pow(2, 261, B.R)
    assert is_zero(reduced(B.limbs(0))) and not is_zero(reduced(one))
    assert is_zero(reduced(B.limbs(B.R))) and is_zero(reduced(B.limbs(8 * B.R)))
    # selector times value, as a program multiplies them: 0 * v is zero, 1 * v is v
    v = rng.randrange(1, B.R)
    z, _w = B.f29_mul(B.limbs(0), B.limbs(v))
    assert is_zero(reduced(z))
    z, _w = B.f29_mul(one, B.limbs(v))
    assert not is_zero(reduced(z))
