"""What the library derives from an AIR descriptor without evaluating a trace
-- the constraint count, every constraint's degree, the quotient degree and what
each constraint is -- against the independent references: oracle/pyoracle.py
(constraint_degrees, log_quotient_degree) and air.py's constraint_names for the
built-in configs, tests/air_program_ref.py's degree rule for a program's part.
The library computes all four by running LineaAIR::eval over a degree algebra
(csrc/air_walk.hpp); the references write the formulas out by hand."""
import ctypes
import itertools
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import air_program_ref as pref  # noqa: E402
import check_constraints_ref as ref  # noqa: E402
from linea_stark_prover_amd.air import (AirLookupConfig, AirPermutationConfig, AirProgramConfig,  # noqa: E402
                                        LineaAIR)

KINDS = {0: "b_inverse", 1: "a_inverse", 2: "first_row", 3: "transition", 4: "last_row"}
TYPES = {1: "permutation", 2: "lookup"}


def perm(na, nb, at=0):
    ids = iter(range(at, at + na + nb + 2))
    take = lambda n: [next(ids) for _ in range(n)]  # noqa: E731
    return AirPermutationConfig(take(na), take(nb), next(ids), next(ids))


def lookup(na, ntab, nbc, at=0):
    ids = iter(range(at, at + na + ntab * (nbc + 3) + 3))
    take = lambda n: [next(ids) for _ in range(n)]  # noqa: E731
    a, b = take(na), [take(nbc) for _ in range(ntab)]
    return AirLookupConfig(a, b, next(ids), take(ntab), next(ids), take(ntab), take(ntab), next(ids))


def _airs():
    out = {}
    for na, nb in itertools.product((1, 2, 3, 6), repeat=2):
        out[f"perm{na}x{nb}"] = LineaAIR([perm(na, nb)])
    for na, ntab, nbc in itertools.product((1, 3), (1, 2, 3), (1, 2, 3)):
        out[f"lookup{na}-{ntab}x{nbc}"] = LineaAIR([lookup(na, ntab, nbc)])
    # two configs, both built-ins, in either order (the second one's columns follow the first's)
    first = lookup(3, 2, 1)
    out["lookup+perm"] = LineaAIR([first, perm(1, 6, at=first.width())])
    first = perm(6, 2)
    out["perm+lookup"] = LineaAIR([first, lookup(1, 3, 2, at=first.width())])
    # a program among the built-ins: degrees 1 + 1, 0 + 2 and one that depends on public_degree
    b = pref.ProgramBuilder(2)
    b.when_first_row().assert_eq(b.local[0], b.public[2], "starts at a public value")
    b.when_transition().assert_eq(b.next[1], b.local[0] * b.local[1], "product")
    b.assert_zero(b.public[0] * b.public[1] * b.local[0] - b.local[1], "public squared")
    out["perm+program+lookup"] = LineaAIR([perm(2, 3), b.build(), lookup(3, 2, 2)])
    return out


AIRS = _airs()


def _expected(air, pd):
    """every constraint's degree from the references, config by config"""
    degs = []
    for c in air.configs:
        if isinstance(c, AirProgramConfig):
            degs += pref.program_degrees(c, pd)
        else:
            degs += ref.O.constraint_degrees(ref.oracle_cfgs(LineaAIR([c])), pd)
    return degs


@pytest.mark.parametrize("pd", [0, 1, 2, 3])
@pytest.mark.parametrize("name", list(AIRS))
def test_derived_quantities_match_the_references(product_lib, name, pd):
    from linea_stark_prover_amd import _lib as L
    lib, air = L.lib(), AIRS[name]
    d = air.descriptor()
    desc, n = (ctypes.c_int32 * len(d))(*d), len(d)
    degs = _expected(air, pd)
    if not any(isinstance(c, AirProgramConfig) for c in air.configs):  # the oracle on the whole AIR at once
        assert degs == ref.O.constraint_degrees(ref.oracle_cfgs(air), pd)
    out = ctypes.c_uint32()
    L.check(lib.lsp_air_num_constraints(desc, n, ctypes.byref(out)))
    assert out.value == len(degs) == len(air.constraint_names())
    got = []
    for j in range(len(degs)):
        L.check(lib.lsp_air_constraint_degree(desc, n, pd, j, ctypes.byref(out)))
        got.append(out.value)
    assert got == degs
    assert lib.lsp_air_constraint_degree(desc, n, pd, len(degs), ctypes.byref(out)) == L.LSP_E_ARG
    L.check(lib.lsp_log_quotient_degree(desc, n, pd, ctypes.byref(out)))
    assert out.value == ref.O.log2_ceil(max(max(degs), 2) - 1)
    if not any(isinstance(c, AirProgramConfig) for c in air.configs):
        assert out.value == ref.O.log_quotient_degree(ref.oracle_cfgs(air), pd)
    for j, want in enumerate(air.constraint_names()):
        cfg, typ, kind, tab = ctypes.c_uint32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        L.check(lib.lsp_air_constraint_info(desc, n, j, ctypes.byref(cfg), ctypes.byref(typ), ctypes.byref(kind),
                                            ctypes.byref(tab)))
        if kind.value == L.LSP_CONSTRAINT_PROGRAM:
            assert typ.value == L.LSP_AIR_PROGRAM and tab.value == -1
            assert want.startswith(f"cfg {cfg.value} program: ")
        else:
            k = KINDS[kind.value] + (f"[{tab.value}]" if tab.value >= 0 else "")
            assert f"cfg {cfg.value} {TYPES[typ.value]}: {k}" == want
            assert (tab.value >= 0) == (typ.value == L.LSP_AIR_LOOKUP and kind.value == L.LSP_CONSTRAINT_B_INVERSE)
    assert lib.lsp_air_constraint_info(desc, n, len(degs), None, None, None, None) == L.LSP_E_ARG
