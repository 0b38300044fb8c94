"""Shared by tests/test_air_program.py and tests/test_gpu_air_program.py: a
big-integer evaluator of LSP_AIR_PROGRAM configs (the independent reference
for AIRs the oracle does not know), the degree rule of include/lsp.h in Python,
and a few small AIRs with their traces.  Nothing here calls the library."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from linea_stark_prover_amd.air import AirProgramConfig, LineaAIR, ProgramBuilder  # noqa: E402
from linea_stark_prover_amd.field import MODULUS, to_mont  # noqa: E402

R = MODULUS


def eval_program(cfg, loc, nxt, pub, first, last, trans):
    """every ASSERT_ZERO's value mod r, in order, as Python ints"""
    slot = [None] * 16
    out = []

    def opnd(x):
        kind, v = x >> 24, x & 0xFFFFFF
        if kind == 0:
            assert slot[v] is not None, "slot read before it is written"
            return slot[v]
        return {1: lambda: loc[v], 2: lambda: nxt[v], 3: lambda: pub[v], 4: lambda: cfg.consts[v],
                5: lambda: first, 6: lambda: last, 7: lambda: trans}[kind]()

    for code, dst, a, b in cfg.ops:
        if code == 4:
            out.append(opnd(a) % R)
        else:
            x, y = opnd(a), opnd(b)
            slot[dst] = (x + y if code == 1 else x - y if code == 2 else x * y) % R
    return out


def eval_air(air, loc, nxt, pub, first, last, trans):
    out = []
    for c in air.configs:
        assert isinstance(c, AirProgramConfig)
        out += eval_program(c, loc, nxt, pub, first, last, trans)
    return out


def program_degrees(cfg, pd):
    """main variable 1, constant 0, public pd, first / last selector 1,
    transition selector 0; Add / Sub max, Mul sum -- per assert"""
    slot = [0] * 16
    leaf = {1: 1, 2: 1, 3: pd, 4: 0, 5: 1, 6: 1, 7: 0}
    out = []

    def deg(x):
        return slot[x & 0xFFFFFF] if x >> 24 == 0 else leaf[x >> 24]

    for code, dst, a, b in cfg.ops:
        if code == 4:
            out.append(deg(a))
        else:
            slot[dst] = deg(a) + deg(b) if code == 3 else max(deg(a), deg(b))
    return out


def report(air, rows, pub, cap):
    """tests/check_constraints_ref.py oracle_report's shape, from eval_air"""
    h = len(rows)
    ncons = len(eval_air(air, rows[0], rows[0], pub, 0, 0, 0))
    counts, first_rows, details, failed = [0] * ncons, [None] * ncons, [], 0
    for i in range(h):
        v = eval_air(air, rows[i], rows[(i + 1) % h], pub, int(i == 0), int(i == h - 1), int(i != h - 1))
        bad = [j for j in range(ncons) if v[j]]
        failed += bool(bad)
        for j in bad:
            counts[j] += 1
            if first_rows[j] is None:
                first_rows[j] = i
            if len(details) < cap:
                details.append((i, j, v[j]))
    first = None
    if failed:
        r = min(x for x in first_rows if x is not None)
        first = (r, min(j for j in range(ncons) if first_rows[j] == r))
    return dict(ok=failed == 0, failed_rows=failed, violations=sum(counts), first=first, counts=counts,
                first_rows=first_rows, details=details)


def rows_to_trace(rows):
    h, w = len(rows), len(rows[0])
    return to_mont([x for r in rows for x in r]).reshape(h, w, 4)


# ------------------------------------------------------------------- AIRs
def fibonacci_air():
    """columns (a, b); public values [alpha, delta, a0, result]: a starts at
    a0 and b at 1, (a, b) -> (b, a + b), the last b is the result.  Degree 2
    (a selector times a difference), so log_q = 0: one quotient chunk."""
    b = ProgramBuilder(2)
    b.when_first_row().assert_eq(b.local[0], b.public[2], "a starts at a0")
    b.when_first_row().assert_eq(b.local[1], 1, "b starts at 1")
    b.when_transition().assert_eq(b.next[0], b.local[1], "a' = b")
    b.when_transition().assert_eq(b.next[1], b.local[0] + b.local[1], "b' = a + b")
    b.when_last_row().assert_eq(b.local[1], b.public[3], "result")
    return LineaAIR([b.build()])


def fibonacci_rows(h, a0=3):
    rows, a, b = [], a0, 1
    for _ in range(h):
        rows.append([a, b])
        a, b = b, (a + b) % R
    return rows, [a0, rows[-1][1]]


def sbox_air(d, c=7):
    """one column: x' = x^d + c, x starts at public value 2 (npub = 3)"""
    b = ProgramBuilder(1)
    x = b.local[0]
    p, e, sq = None, d, x
    while e:
        if e & 1:
            p = sq if p is None else p * sq
        e >>= 1
        if e:
            sq = sq * sq
    b.when_first_row().assert_eq(x, b.public[2], "x starts at x0")
    b.when_transition().assert_eq(b.next[0], p + c, f"x' = x^{d} + c")
    return LineaAIR([b.build()])


def sbox_rows(h, d, c=7, x0=5):
    rows, x = [], x0
    for _ in range(h):
        rows.append([x])
        x = (pow(x, d, R) + c) % R
    return rows, [x0]


def pressure_air(nslots):
    """two asserts that keep exactly `nslots` values live: the n = nslots - 1
    products t_i = x_i x_i' are shared by a forward and a backward sum, so all
    of them stay in slots beside the first sum's accumulator.  Public value 2
    is the sum's value."""
    n = nslots - 1
    assert n >= 2
    b = ProgramBuilder(n)
    t = [b.local[i] * b.next[i] for i in range(n)]
    s = t[0]
    for x in t[1:]:
        s = s + x
    u = t[n - 1]
    for x in reversed(t[:n - 1]):
        u = u + x
    b.assert_eq(s, b.public[2], "forward sum")
    b.assert_eq(u, b.public[2], "backward sum")
    cfg = b.build()
    assert cfg.nslots == nslots, cfg.nslots
    return LineaAIR([cfg])


def pressure_rows(h, nslots):
    """x_i = (i + 2) on even rows and -(i + 2) on odd ones: every product of a
    row with its successor (cyclically, h even) is -(i + 2)^2"""
    n = nslots - 1
    rows = [[(i + 2) * (1 if j % 2 == 0 else -1) % R for i in range(n)] for j in range(h)]
    return rows, [-sum((i + 2) ** 2 for i in range(n)) % R]


def long_air(nops=2000, z=3):
    """about `nops` ops on one column: a Horner chain in the constant z (so the
    degree stays 2), its value pinned by public value 2 (see long_rows)"""
    b = ProgramBuilder(1)
    acc = b.local[0]
    k = 0
    while 2 * k + 4 < nops:
        acc = acc * z + (k + 1)
        k += 1
    b.assert_eq(acc * b.local[0], b.public[2] * b.local[0], "chain")
    return LineaAIR([b.build()]), k


def long_rows(h, k, z=3, x=11):
    """every row holds x; public value: chain(x)"""
    acc = x
    for i in range(k):
        acc = (acc * z + i + 1) % R
    return [[x] for _ in range(h)], [acc]


def slotless_air():
    """an assert of LOCAL directly: 0 slots"""
    b = ProgramBuilder(2)
    b.assert_zero(b.local[1], "column 1 is zero")
    return LineaAIR([b.build()])
