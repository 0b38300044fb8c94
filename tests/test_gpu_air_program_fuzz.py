"""The program interpreter of k_air_prog.hpp against the big-integer evaluator
on the fuzz corpus of tests/air_program_fuzz.py: raw programs in the op forms
ProgramBuilder never emits, on edge-laden cells, constants and public values,
through k_check<true> / k_check_rows<true> (check_constraints), through
k_quotient<EARLY, true> (quotient_values, whole proofs under both settings of
LSP_QUOTIENT_EARLY) and through the debug-bounds build.  Every comparison is
exact, and every device result is held to the evaluator or to the host
verifier, never to another device run alone."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import air_program_fuzz as F  # noqa: E402
import check_constraints_ref as ref  # noqa: E402
from linea_stark_prover_amd.field import from_mont, to_mont  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)
R = F.R
CORPUS = F.corpus()
LARGE = F.large_subset()
FAMILIES = ["free", "identity", "solvable"]
ALPHA = 0xabcdef0123456789 * 0x1000193 + 11


@pytest.fixture(scope="module")
def pubs(gpu_ctx):
    a, d, _ = gpu_ctx.config.seeded()
    return from_mont(np.concatenate([a, d]))


def _check(gpu_ctx, case, rows, pubi, prows):
    pre = F.to_matrix(prows) if prows is not None else None
    return ref.as_dict(gpu_ctx.check_constraints(F.to_matrix(rows), case.air, to_mont(pubi), max_violations=64,
                                                 preprocessed=pre))


def _check_case(gpu_ctx, case, h, pubs):
    pubi = pubs + case.extra
    rows, prows = case.rows(h, pubi), case.prows(h)
    exp = F.report(case.air, rows, pubi, 64, prows)
    got = _check(gpu_ctx, case, rows, pubi, prows)
    assert got == exp, (case, h)
    if case.family == "identity":
        assert got["ok"] and got["failed_rows"] == 0, (case, h)
    return exp


# ------------------------------------------------------------------- check
@pytest.mark.parametrize("family", FAMILIES)
def test_check_equals_the_evaluator(gpu_ctx, pubs, family):
    """h = 8: a partial wave, whose dead lanes walk row 0"""
    bad = 0
    for case in CORPUS:
        if case.family == family:
            bad += not _check_case(gpu_ctx, case, 8, pubs)["ok"]
    # the reports compared are not all empty: free programs and the random
    # permutation columns of the multi-config cases break nearly every row
    assert bad >= (50 if family == "free" else 0)


@pytest.mark.parametrize("case", LARGE, ids=[c.name for c in LARGE])
def test_check_equals_the_evaluator_over_several_blocks(gpu_ctx, pubs, case):
    """h = 512: two blocks of 256 threads or four of 128; the counts and first
    rows come through atomics of several waves, the 64 listed values from rows
    of one (free programs) or of several (a few broken cells) waves"""
    _check_case(gpu_ctx, case, 512, pubs)
    if case.family == "free":
        return
    # a satisfied (or identically zero) program with cells broken in five waves
    pubi = pubs + case.extra
    perm = None
    if len(case.parts) > 1:
        from linea_stark_prover_amd.prover import gen_permutation_trace
        a, d = to_mont(pubs[:1]), to_mont(pubs[1:2])
        perm = ref.ints(gen_permutation_trace(9, case.parts[1][1], a, d))
    rows, prows = case.rows(512, pubi, perm), case.prows(512)
    rng = random.Random(case.seed)
    for r_ in (0, 63, 64, 200, 300, 450, 511):
        c = rng.randrange(case.width)
        rows[r_][c] = (rows[r_][c] + 1 + rng.randrange(3)) % R
    exp = F.report(case.air, rows, pubi, 64, prows)
    assert _check(gpu_ctx, case, rows, pubi, prows) == exp
    assert exp["ok"] == (case.family == "identity")


# ---------------------------------------------------------------- quotient
def _quotient_case(gpu_ctx, case, h, pubs):
    """the LDE need not be one: the kernel reads rows, so a random edge-laden
    N x w matrix stands for the columns on the coset"""
    lb = gpu_ctx.config.log_blowup
    N = h << lb
    pubi = pubs + case.extra
    rng = random.Random(case.seed * 31337 + h)
    ev = F.draw_rows(rng, N, case.width)
    pev = F.draw_rows(rng, N, case.prep_width) if case.prep_width else None
    log_q = case.log_q()
    exp = F.quotient_ref(case.air, ev, h, log_q, pubi, ALPHA, pev)
    got = gpu_ctx.quotient_values(F.to_lde(ev), h, case.air, to_mont(pubi), to_mont([ALPHA]),
                                  prep_lde=F.to_lde(pev) if pev else None)
    assert got.shape == (h << log_q, 4)
    assert from_mont(got) == exp, (case, h)
    if case.family == "identity":
        assert not got.any(), (case, h)  # canonical zero: the all-zero words, not r
    return exp


@pytest.mark.parametrize("family", FAMILIES)
def test_quotient_values_equal_the_evaluator(gpu_ctx, pubs, family):
    """h = 4: at most 32 points, a partial wave"""
    nonzero = 0
    for case in CORPUS:
        if case.family == family:
            nonzero += any(_quotient_case(gpu_ctx, case, 4, pubs))
    assert nonzero >= (50 if family == "free" else 20 if family == "solvable" else 0)


@pytest.mark.parametrize("case", LARGE, ids=[c.name for c in LARGE])
def test_quotient_values_equal_the_evaluator_over_several_blocks(gpu_ctx, pubs, case):
    """h = 64: up to 512 points, several blocks in both block forms"""
    _quotient_case(gpu_ctx, case, 64, pubs)


# ------------------------------------------------------------ whole proofs
PROVABLE = [c for c in CORPUS if c.family == "solvable"] + [c for c in CORPUS if c.name == "identity12"]


@pytest.mark.parametrize("log_h", [4, 8])
def test_proofs_verify_under_both_quotient_paths(gpu_ctx, pubs, monkeypatch, log_h):
    """the host verifier's evaluation of the program at zeta is the reference;
    the fold of the stored constraint values (LSP_QUOTIENT_EARLY=1) and the
    fold in the walker give the same bytes on top of that"""
    from linea_stark_prover_amd.prover import gen_permutation_trace
    h = 1 << log_h
    a, d = to_mont(pubs[:1]), to_mont(pubs[1:2])
    assert any(len(c.parts) > 1 for c in PROVABLE) and any(c.family == "identity" for c in PROVABLE)
    for case in PROVABLE:
        pubi = pubs + case.extra
        pub = to_mont(pubi)
        perm = None
        if len(case.parts) > 1 and isinstance(case.parts[1], tuple):
            perm = ref.ints(gen_permutation_trace(log_h, case.parts[1][1], a, d))
        rows, prows = case.rows(h, pubi, perm), case.prows(h)
        assert F.report(case.air, rows, pubi, 4, prows)["ok"], case
        pre = gpu_ctx.preprocess(F.to_matrix(prows)) if prows is not None else None
        trace = F.to_matrix(rows)
        proofs = []
        for early in ("0", "1"):
            monkeypatch.setenv("LSP_QUOTIENT_EARLY", early)
            proofs.append(gpu_ctx.prove(trace, case.air, pub, preprocessed=pre))
        assert proofs[0] == proofs[1], (case, h)
        assert gpu_ctx.verify(proofs[0], case.air, pub, preprocessed=pre), (case, h)
        bad = list(pubi)
        bad[2] = (bad[2] + 1) % R
        assert not gpu_ctx.verify(proofs[0], case.air, to_mont(bad), preprocessed=pre), (case, h)


# ------------------------------------------------------- debug-bounds build
DBG_CASES = [c.name for c in LARGE if c.family != "solvable"] + ["multi0", "nconst1"]

CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import air_program_fuzz as F
import check_constraints_ref as ref
import test_gpu_air_program_fuzz as T
from linea_stark_prover_amd import _lib as L
from linea_stark_prover_amd.field import from_mont
from linea_stark_prover_amd.prover import Context, StarkConfig
assert b"debug-bounds" in L.lib().lsp_version()
names = sys.argv[2].split(",")
cases = [c for c in F.corpus() if c.name in names]
assert len(cases) == len(names) == 10
assert {F.regime(c.nslots) for c in cases} == set(F.REGIMES) and any(len(c.parts) > 1 for c in cases)
with Context(StarkConfig()) as ctx:
    a, d, _ = ctx.config.seeded()
    pubs = from_mont(np.concatenate([a, d]))
    for c in cases:
        for h in (8, 512):
            T._check_case(ctx, c, h, pubs)
        for h in (4, 64):
            T._quotient_case(ctx, c, h, pubs)
print("debug-bounds ok")
'''


def test_debug_bounds_build_reports_no_failed_check_on_the_corpus():
    """ten corpus programs spanning the four regimes and two multi-config
    descriptors through check and quotient: a fired LSP_BOUNDS probe fails the
    call (LSP_E_STATE), and the results still equal the evaluator's"""
    from linea_stark_prover_amd import build as B
    assert os.path.exists(B.DBG_LIB), "liblsp_hip_dbg.so not built (python -m linea_stark_prover_amd.build --debug-bounds)"
    env = dict(os.environ, LSP_LIB=B.DBG_LIB)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, ",".join(DBG_CASES)], env=env, capture_output=True,
                       text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "debug-bounds ok" in r.stdout
