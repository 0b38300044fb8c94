"""The expected report of check_constraints from the Python oracle alone
(oracle/pyoracle.py eval_constraints, called per row with 0/1 selectors), shared
by tests/test_check_constraints.py and tests/test_gpu_check_constraints.py.
Nothing here calls the code under test except the trace generators."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from linea_stark_prover_amd.air import AirPermutationConfig  # noqa: E402
from linea_stark_prover_amd.field import MODULUS, from_mont, to_mont  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

# the reduced wide AIR: 2 lookups (2-column A, two 2-column tables) then 2
# permutation groups of 3 + 3 columns -- both config types, a table index > 0
MIXED = dict(nlookup=2, na=2, ntab=2, nperm=2, pcols=3)


def oracle_cfgs(air):
    out = []
    for c in air.configs:
        if isinstance(c, AirPermutationConfig):
            out.append(O.PermCfg(list(c.a_columns_ids), list(c.b_columns_ids), c.b_inverse_id, c.check_id))
        else:
            out.append(O.LookupCfg(list(c.a_columns_ids), [list(t) for t in c.b_columns_ids], c.a_filter_id,
                                   list(c.b_filter_id), c.a_inverses_id, list(c.b_inverses_id),
                                   list(c.occurrences_id), c.check_id))
    return out


def ints(trace):
    """(h, w, 4) Montgomery limbs -> h lists of w ints"""
    h, w = trace.shape[0], trace.shape[1]
    flat = from_mont(trace.reshape(-1, 4))
    return [flat[i * w:(i + 1) * w] for i in range(h)]


def oracle_report(air, rows, alpha, delta, cap):
    """rows: h lists of w ints.  The whole report: summary, every count, every
    first row, the first `cap` violations in (row, constraint) order with values."""
    cfgs = oracle_cfgs(air)
    h = len(rows)
    ncons = len(O.eval_constraints(cfgs, rows[0], rows[0], alpha, delta, 0, 0, 0))
    counts, first_rows, details = [0] * ncons, [None] * ncons, []
    failed = 0
    for i in range(h):
        v = O.eval_constraints(cfgs, rows[i], rows[(i + 1) % h], alpha, delta, int(i == 0), int(i == h - 1),
                               int(i != h - 1))
        bad = [j for j in range(ncons) if v[j] % MODULUS]
        failed += bool(bad)
        for j in bad:
            counts[j] += 1
            if first_rows[j] is None:
                first_rows[j] = i
            if len(details) < cap:
                details.append((i, j, v[j] % MODULUS))
    first = None
    if failed:
        r = min(x for x in first_rows if x is not None)
        first = (r, min(j for j in range(ncons) if first_rows[j] == r))
    return dict(ok=failed == 0, failed_rows=failed, violations=sum(counts), first=first, counts=counts,
                first_rows=first_rows, details=details)


def cut(exp, cap):
    """an oracle_report made with a larger cap, its detail list cut to `cap`"""
    return dict(exp, details=exp["details"][:cap])


def as_dict(report):
    """a ConstraintReport in oracle_report's shape"""
    for v in report.details:
        assert v.name == report.names[v.index]
    return dict(ok=report.ok, failed_rows=report.failed_rows, violations=report.violations, first=report.first,
                counts=list(report.counts), first_rows=list(report.first_rows),
                details=[(v.row, v.index, v.value) for v in report.details])


def tamper(trace, rows, r, c):
    """add 1 to cell (r, c) of both the limb array and the int rows (copies)"""
    t = trace.copy()
    rr = [list(x) for x in rows]
    rr[r][c] = (rr[r][c] + 1) % MODULUS
    t[r, c] = to_mont([rr[r][c]])[0]
    return t, rr


def column_classes(air):
    """one column per class of the issue's list, from the last permutation and
    the last lookup config of `air` (so ids are shifted), table 1 where a class
    has tables: name -> column id"""
    out = {}
    perm = [c for c in air.configs if isinstance(c, AirPermutationConfig)]
    look = [c for c in air.configs if not isinstance(c, AirPermutationConfig)]
    if perm:
        p = perm[-1]
        out.update({"perm.a": p.a_columns_ids[0], "perm.b": p.b_columns_ids[-1], "perm.b_inverse": p.b_inverse_id,
                    "perm.check": p.check_id})
    if look:
        k = look[-1]
        out.update({"lookup.a": k.a_columns_ids[0], "lookup.b[1]": k.b_columns_ids[1][0],
                    "lookup.a_filter": k.a_filter_id, "lookup.b_filter[1]": k.b_filter_id[1],
                    "lookup.a_inverses": k.a_inverses_id, "lookup.b_inverses[1]": k.b_inverses_id[1],
                    "lookup.occurrences[1]": k.occurrences_id[1], "lookup.check": k.check_id})
    return out


def pub_ints(pub):
    a, d = from_mont(np.asarray(pub).reshape(-1, 4)[:2])
    return a, d
