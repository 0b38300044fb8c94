"""Witness inputs with one zero denominator (row combination + delta = 0),
shared by tests/test_gpu_inverse_zeros.py (the device must refuse them) and
tests/test_inverse_zeros_oracle.py (the reference's restatement refuses them).

Every block has single-column rows or a last column solved for, so a cell can
be set to make its row combination equal -delta.  Apart from that cell each
input is a valid lookup / permutation, and `good` is the same input without it.
"""
import functools

from oracle import pyoracle as O

P = O.P
LOOKUP_SIZES = (8, 4096)      # 2 n elements in one batch: the base kernel, and one up/down level
LOOKUP_SPOTS = ("table_enabled", "table_disabled", "a_enabled", "a_disabled")
PERM_SIZES = (8, 4096)


@functools.lru_cache(maxsize=None)
def challenges():
    s = O.setup_from_seed()
    return s.alpha, s.delta


def zero_row(n):
    """the row that gets the zero denominator: neither end, not a multiple of the kernels' 256"""
    return (5 * n) // 8 + 1


def lookup_case(n, spot):
    """(good, bad): each (a, b, a_filter, b_filter) with na = nbc = 1 and one
    table.  The table holds 1..n; A row i looks up 1 + (3 i mod n/2), so the
    table's upper half is never looked up and a cell there can change freely.
    Rows n/4 of A and 3n/4 + 1 of the table are disabled."""
    _, delta = challenges()
    tab = [1 + i for i in range(n)]
    a = [1 + (3 * i) % (n // 2) for i in range(n)]
    af, bf = [1] * n, [1] * n
    af[n // 4] = 0
    a[n // 4] = 5 * n  # a disabled A row may hold what no table has
    bf[3 * n // 4 + 1] = 0
    good = ([list(a)], [[list(tab)]], list(af), [list(bf)])
    r = zero_row(n)  # in the upper half
    kind, state = spot.split("_")
    col, fil = (tab, bf) if kind == "table" else (a, af)
    col[r] = (-delta) % P
    fil[r] = int(state == "enabled")
    return good, ([a], [[tab]], af, [bf])


def perm_case(n):
    """(good, bad): each (a, b) of two columns, b = a's rows rotated by 3; in
    `bad` one row's second cell is solved for, so that this row's combination
    is -delta -- in A and, three rows on, in B: still a permutation."""
    alpha, delta = challenges()
    rng = O.SplitMix64(n)
    a = [[rng.sample_fr() for _ in range(n)] for _ in range(2)]
    rot = lambda c: c[3:] + c[:3]  # noqa: E731
    good = ([list(c) for c in a], [rot(c) for c in a])
    r = zero_row(n)
    a[1][r] = (-delta - a[0][r] * alpha) % P
    return good, (a, [rot(c) for c in a])
