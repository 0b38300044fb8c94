"""check_constraints on the GPU (k_check.hip behind lsp_check_constraints)
against oracle/pyoracle.py eval_constraints called per row with 0/1 selectors:
the whole report -- summary, every count, every first row, the detail list
with values -- at the smallest shapes where the kernel's own machinery can go
wrong (a partial wave, one wave and one mask word, `next` across a wave and a
mask word, across a block, many blocks with contended counters), from a host
array and from a device pointer; against the library's host path where the
Python oracle is too slow (2^14 x 184); through prove(check=True), the
LSP_CHECK_CONSTRAINTS=1 switch of lsp_prove in a fresh process, and the
bounds-checked debug library."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import check_constraints_ref as ref  # noqa: E402
from linea_stark_prover_amd.air import permutation_air  # noqa: E402
from linea_stark_prover_amd.field import MODULUS, to_mont  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(gpu_ctx):
    from linea_stark_prover_amd import prover as P
    a, d, _ = gpu_ctx.config.seeded()
    pub = np.concatenate([a, d])
    alpha, delta = ref.pub_ints(pub)
    cache = {}

    def traces(log_n):
        if log_n not in cache:
            tp = P.gen_permutation_trace(log_n, 3, a, d)
            tm, am = P.gen_wide_trace(log_n, a, d, **ref.MIXED)
            cache[log_n] = {"perm": (tp, permutation_air(3), ref.ints(tp)), "mixed": (tm, am, ref.ints(tm))}
        return cache[log_n]

    return dict(P=P, ctx=gpu_ctx, pub=pub, alpha=alpha, delta=delta, a=a, d=d, traces=traces)


def _check(env, trace, air, pub, cap, device_ptr):
    ctx = env["ctx"]
    if not device_ptr:
        return ctx.check_constraints(trace, air, pub, max_violations=cap)
    t = np.ascontiguousarray(trace)
    p = ctx.dev_alloc(t.nbytes)
    try:
        ctx.h2d(p, t)
        return ctx.check_constraints(p, air, pub, h=t.shape[0], w=t.shape[1], max_violations=cap)
    finally:
        ctx.dev_free(p)


# log_n, which AIR, device pointer?, the tampered cells (row, column class)
SHAPES = [
    (1, "perm", False, [(0, "perm.check")]),                       # a partial wave; first and last adjacent; wrap
    (1, "mixed", True, [(1, "lookup.a_inverses")]),
    (1, "mixed", False, [(1, "lookup.check"), (0, "perm.b")]),
    (6, "perm", True, [(63, "perm.check")]),                       # one wave, one mask word
    (6, "mixed", False, [(0, "lookup.check"), (62, "lookup.b[1]"), (63, "perm.b_inverse")]),
    (7, "mixed", False, [(63, "perm.check"), (64, "lookup.check")]),   # next crosses a wave and a mask word
    (7, "perm", True, [(63, "perm.b_inverse"), (64, "perm.a")]),
    (9, "mixed", True, [(255, "lookup.check"), (256, "perm.check"), (511, "lookup.occurrences[1]")]),  # block edge
    (9, "perm", False, [(255, "perm.check"), (256, "perm.check"), (511, "perm.check")]),
    (12, "mixed", True, [(0, "perm.check"), (1000, "lookup.a_filter"), (2047, "lookup.b_inverses[1]"),
                         (2048, "perm.a"), (4095, "lookup.check")]),   # many blocks
]
IDS = [f"2^{s[0]}-{s[1]}-{'dev' if s[2] else 'host'}" for s in SHAPES]


@pytest.mark.parametrize("log_n,which,dev,cells", SHAPES, ids=IDS)
def test_valid_tampered_and_wrong_challenges(env, log_n, which, dev, cells):
    trace, air, rows = env["traces"](log_n)[which]
    h = len(rows)
    alpha, delta, pub = env["alpha"], env["delta"], env["pub"]
    # valid
    exp = ref.oracle_report(air, rows, alpha, delta, 16)
    assert exp["ok"]
    rep = _check(env, trace, air, pub, 16, dev)
    assert ref.as_dict(rep) == exp and rep.ok and rep.details == []
    # tampered cells, every violation listed
    cols = ref.column_classes(air)
    t, rr = trace, rows
    for r_, cls in cells:
        t, rr = ref.tamper(t, rr, r_, cols[cls])
    exp = ref.oracle_report(air, rr, alpha, delta, 4096)
    assert not exp["ok"] and exp["violations"] < 4096
    assert ref.as_dict(_check(env, t, air, pub, 4096, dev)) == exp
    # ... and the list cut short
    assert ref.as_dict(_check(env, t, air, pub, 1, not dev)) == ref.cut(exp, 1)
    assert ref.as_dict(_check(env, t, air, pub, 0, dev)) == ref.cut(exp, 0)
    # the wrong challenges: every row fails every inverse constraint (contended counters, atomicMin first rows)
    a2, d2 = (alpha + 1) % MODULUS, (delta + 5) % MODULUS
    exp = ref.oracle_report(air, rows, a2, d2, 40)
    rep = _check(env, trace, air, to_mont([a2, d2]), 40, dev)
    assert ref.as_dict(rep) == exp
    inv = [j for j, n in enumerate(rep.names) if "inverse" in n]
    assert inv and all(rep.counts[j] == h and rep.first_rows[j] == 0 for j in inv) and rep.failed_rows == h


def test_gpu_report_equals_host_path_on_the_wide_trace(env):
    """2^14 x 184, the default wide AIR (56 constraints): valid (no false
    positive of the zero test in ~10^6 constraint evaluations), 5 scattered
    tampered cells, wrong challenges -- GPU report == host-path report"""
    P = env["P"]
    trace, air = P.gen_wide_trace(14, env["a"], env["d"])
    h, w = trace.shape[0], trace.shape[1]
    assert (h, w) == (1 << 14, 184) and len(air.constraint_names()) == 56
    host = P.Context(P.StarkConfig(), device=-1)
    p = env["ctx"].dev_alloc(trace.nbytes)
    try:
        def both(pub, cap):
            env["ctx"].h2d(p, trace)
            g = env["ctx"].check_constraints(p, air, pub, h=h, w=w, max_violations=cap)
            c = host.check_constraints(trace, air, pub, max_violations=cap)
            assert ref.as_dict(g) == ref.as_dict(c) and g.names == c.names
            return g

        g = both(env["pub"], 64)
        assert g.ok and g.violations == 0 and not any(g.counts)
        one = to_mont([1])[0]
        rng = np.random.RandomState(5)
        for r_, c_ in zip([0, 4095, 4096, 9999, h - 1], rng.randint(0, w, 5)):
            trace[r_, c_] = one if not np.array_equal(trace[r_, c_], one) else to_mont([2])[0]
        g = both(env["pub"], 64)
        assert not g.ok and 1 <= g.failed_rows <= 10 and len(g.details) == g.violations
        g = both(to_mont([env["alpha"] + 1, env["delta"] + 5]), 100)
        assert g.failed_rows == h and len(g.details) == 100 and g.first == (0, 0)
    finally:
        env["ctx"].dev_free(p)
        host.close()


def test_prove_check(env):
    P, ctx = env["P"], env["ctx"]
    trace, air, rows = env["traces"](10)["mixed"]
    ok = ctx.prove(trace, air, env["pub"], check=True)
    assert ok == ctx.prove(trace, air, env["pub"], check=False) == ctx.prove(trace, air, env["pub"])
    assert ctx.verify(ok, air, env["pub"])
    t, rr = ref.tamper(trace, rows, 517, ref.column_classes(air)["lookup.check"])
    exp = ref.oracle_report(air, rr, env["alpha"], env["delta"], 16)
    with pytest.raises(P.ConstraintError) as e:
        ctx.prove(t, air, env["pub"], check=True)
    assert e.value.report.first == exp["first"] and ref.as_dict(e.value.report) == exp
    with pytest.raises(P.ConstraintError):
        P.prove(ctx.config, air, t, env["pub"], ctx=ctx, check=True)


CHILD_ENV = r'''
import ctypes, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import check_constraints_ref as ref
from linea_stark_prover_amd import _lib as L
from linea_stark_prover_amd import prover as P
os.environ.pop("LSP_CHECK_CONSTRAINTS", None)
ctx = P.Context(P.StarkConfig())
a, d, _ = ctx.config.seeded()
pub = np.concatenate([a, d])
alpha, delta = ref.pub_ints(pub)
trace, air = P.gen_wide_trace(10, a, d, **ref.MIXED)
rows = ref.ints(trace)
desc = (ctypes.c_int32 * len(air.descriptor()))(*air.descriptor())

def c_prove(t):
    t = np.ascontiguousarray(t)
    proof = ctypes.c_void_p()
    rc = L.lib().lsp_prove(ctx.h, t.ctypes.data, t.shape[0], t.shape[1], desc, len(desc), pub.ctypes.data, 2,
                           L.LSP_MEM_HOST, ctypes.byref(proof))
    return rc, (P._take_proof(proof) if rc == 0 else L.lib().lsp_last_error(ctx.h).decode())

rc, plain = c_prove(trace)
assert rc == 0
bad, rr = ref.tamper(trace, rows, 700, ref.column_classes(air)["lookup.b_inverses[1]"])
rc, unchecked = c_prove(bad)
assert rc == 0 and not ctx.verify(unchecked, air, pub)   # unset: a bad trace is proved, as before
os.environ["LSP_CHECK_CONSTRAINTS"] = "1"
rc, checked = c_prove(trace)
assert rc == 0 and checked == plain
rc, msg = c_prove(bad)
exp = ref.oracle_report(air, rr, alpha, delta, 0)
r, j = exp["first"]
name = air.constraint_names()[j]            # "cfg C kind: what[T]"
cfg, what = name.split()[1], name.split(": ")[1]
kind = what.split("[")[0] + (", table " + what.split("[")[1][:-1] if "[" in what else "")
want = f"constraints had nonzero value on row {r}: constraint {j} (config {cfg}, {kind}); {exp['failed_rows']} rows fail"
assert rc == L.LSP_E_CONSTRAINT == 7 and msg == want, (rc, msg, want)
os.environ["LSP_CHECK_CONSTRAINTS"] = "0"
assert c_prove(bad)[0] == 0
print("env switch ok:", msg)
'''


def test_env_switch_in_a_fresh_process():
    env_ = {k: v for k, v in os.environ.items() if k != "LSP_CHECK_CONSTRAINTS"}
    r = subprocess.run([sys.executable, "-c", CHILD_ENV, ROOT], env=env_, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "env switch ok: constraints had nonzero value on row " in r.stdout


CHILD_DBG = r'''
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import check_constraints_ref as ref
from linea_stark_prover_amd import _lib as L
from linea_stark_prover_amd import prover as P
assert b"debug-bounds" in L.lib().lsp_version()
with P.Context(P.StarkConfig()) as ctx:
    a, d, _ = ctx.config.seeded()
    pub = np.concatenate([a, d])
    alpha, delta = ref.pub_ints(pub)
    trace, air = P.gen_wide_trace(9, a, d, **ref.MIXED)
    rows = ref.ints(trace)
    assert ref.as_dict(ctx.check_constraints(trace, air, pub)) == ref.oracle_report(air, rows, alpha, delta, 16)
    t, rr = ref.tamper(trace, rows, 511, ref.column_classes(air)["perm.check"])
    assert ref.as_dict(ctx.check_constraints(t, air, pub)) == ref.oracle_report(air, rr, alpha, delta, 16)
print("debug-bounds check ok")
'''


def test_debug_bounds_library():
    """one valid and one tampered trace through liblsp_hip_dbg.so: no bounds check fires"""
    from linea_stark_prover_amd import build as B
    assert os.path.exists(B.DBG_LIB), "liblsp_hip_dbg.so not built (python -m linea_stark_prover_amd.build --debug-bounds)"
    r = subprocess.run([sys.executable, "-c", CHILD_DBG, ROOT], env=dict(os.environ, LSP_LIB=B.DBG_LIB),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "debug-bounds check ok" in r.stdout
