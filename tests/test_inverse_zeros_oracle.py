"""The reference refuses a zero denominator: Field::inverse panics on zero
(trace/src/lookup.rs:126,144 invert every row, disabled ones too;
trace/src/permutation.rs the B rows), and its restatement raises
ZeroDivisionError.  The same inputs must be refused on the device
(tests/test_gpu_inverse_zeros.py)."""
import os
import sys

import pytest

from oracle import pyoracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import inverse_zero_cases as Z  # noqa: E402


@pytest.mark.parametrize("spot", Z.LOOKUP_SPOTS)
@pytest.mark.parametrize("n", Z.LOOKUP_SIZES)
def test_lookup_witness_refuses_zero_denominator(n, spot):
    al, de = Z.challenges()
    good, bad = Z.lookup_case(n, spot)
    with pytest.raises(ZeroDivisionError):
        O.lookup_witness(*bad, al, de)
    if spot == Z.LOOKUP_SPOTS[0]:
        O.lookup_witness(*good, al, de)  # the input is valid but for that cell


@pytest.mark.parametrize("n", Z.PERM_SIZES)
def test_perm_witness_refuses_zero_denominator(n):
    al, de = Z.challenges()
    good, bad = Z.perm_case(n)
    with pytest.raises(ZeroDivisionError):
        O.perm_witness(*bad, al, de)
    O.perm_witness(*good, al, de)
    # but for the division the bad input is a permutation too: the same rows in both
    assert sorted(zip(*bad[0])) == sorted(zip(*bad[1]))
