"""The witness edge cases (tests/witness_cases.py) are what they claim, against
pyoracle alone: the closed forms are the reference's columns, the colliding
keys collide under the model of the kernel's hash, the reference accepts every
case meant to succeed and refuses the one meant to fail, and the generator
model's B is a row shuffle of its A.  The device sees the same cases in
tests/test_gpu_witness_edges.py."""
import os
import sys

import pytest

from oracle import pyoracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import witness_cases as W  # noqa: E402

P = O.P


def test_word_helpers_round_trip():
    for v in (0, 1, 2, P - 1, O.MONT_R % P, W.rand_fr(1, 1)[0]):
        w = W.to_words(v)
        assert W.from_words(w) == v
        assert sum(x << (64 * k) for k, x in enumerate(w)) == v * O.MONT_R % P
    xs = W.rand_fr(2, 9) + [1, P - 1]
    assert [x * y % P for x, y in zip(xs, W.batch_inv(xs))] == [1] * len(xs)


@pytest.mark.parametrize("n", [1, 2, 7, 2049])
def test_rotation_permutation_closed_form(n):
    a, b = W.rotation_perm_input(n)
    cols = W.rotation_perm_columns(n)
    got = W.rotation_perm_rows(lambda i: a[0][i], n, range(n))
    assert got == [[c[i] for c in cols] for i in range(n)]
    assert cols[3][-1] == 1 and b[0][1 % n] == a[0][0]


@pytest.mark.parametrize("n", [1, 2, 7, 2049])
def test_rotation_lookup_closed_form(n):
    a, b, _, _ = W.rotation_lookup_input(n)
    cols = W.rotation_lookup_columns(n)
    got = W.rotation_lookup_rows(lambda i: b[0][0][i], n, range(n))
    assert got == [[c[i] for c in cols] for i in range(n)]
    assert cols[6] == [1] * n and cols[7][-1] == 0


@pytest.mark.parametrize("n", W.PERM_BIG_SIZES + (W.LOOKUP_BIG_SIZE,))
def test_big_rows_cover_the_boundaries(n):
    rows = W.big_rows(n)
    s = set(rows)
    tiles = -(-n // W.SC_TILE)
    assert tiles > W.SC_TILE  # a second level of more than one tile
    assert rows == sorted(s) and rows[0] == 0 and rows[-1] == n - 1 and len(rows) >= 2000
    assert set(range(16)) <= s and set(range(n - 16, n)) <= s
    for k in (1, 2, 2047, 2048, 2049, tiles - 1):
        assert {r for r in (k * 2048 - 1, k * 2048, k * 2048 + 7) if r < n} <= s
    assert (tiles - 1) * 2048 in s  # the last tile's first row
    assert W.big_rows(n) == rows


def test_key_hash_model_reads_words_0_and_2():
    w = (0x1111111111111111, 0x2222222222222222, 0x3333333333333333, 0x0444444444444444)
    h = W.key_hash(w)
    assert 0 <= h < 1 << 32
    assert W.key_hash((w[0], 5, w[2], 6)) == h
    assert W.key_hash((w[0] ^ 1, w[1], w[2], w[3])) != h
    assert W.key_hash((w[0], w[1], w[2] ^ 1, w[3])) != h
    assert [W.occ_capacity(m) for m in (1, 16, 32, 33, 1024, 2 * 4097)] == [64, 64, 64, 128, 2048, 32768]


@pytest.mark.parametrize("count,cap,slot", [(8, 64, 61), (W.CHAIN_KEYS, 2048, W.CHAIN_SLOT)])
def test_colliding_keys(count, cap, slot):
    keys = W.colliding_keys(count, cap, slot)
    assert len(keys) == count
    assert {W.key_hash(k) & (cap - 1) for k in keys} == {slot}
    assert len({W.key_hash(k) for k in keys}) == 1
    assert len({(k[0], k[2]) for k in keys}) == 1
    assert len({k[1] for k in keys}) == count and len({k[3] for k in keys}) == count
    assert all(k[3] < 1 << 58 for k in keys)
    vals = [W.from_words(k) for k in keys]
    assert len(set(vals)) == count and all(W.to_words(v) == k for v, k in zip(vals, keys))
    assert count > cap - slot  # the chain of these keys alone passes the table's last slot


def test_table_cases_use_the_capacity_they_name():
    a, b, _, _ = W.LOOKUP_CASES["wrap8"]()
    assert W.occ_capacity(len(a[0]) * (1 + len(b))) == 64
    a, b, _, _ = W.LOOKUP_CASES["chain300"]()
    assert W.occ_capacity(len(a[0]) * (1 + len(b))) == 2048
    keys = {W.from_words(k) for k in W.colliding_keys(W.CHAIN_KEYS, 2048, W.CHAIN_SLOT)}
    assert keys <= set(b[0][0])
    counts = sorted(a[0].count(k) for k in keys)
    assert counts == [1] * 225 + [3] * 75


def test_high_filters_have_zero_low_words():
    f = W.HIGH_FILTERS
    assert W.to_words(f[0])[:3] == (0, 0, 0) and W.to_words(f[0])[3]
    assert W.to_words(f[1])[:2] == (0, 0) and W.to_words(f[1])[3] == 0 and W.to_words(f[1])[2]
    assert f[2:] == (2, P - 1) and all(0 < x < P for x in f)
    _, _, af, bf = W.LOOKUP_CASES["high_filters"]()
    assert set(f) <= set(af) and set(f) <= set(bf[0]) and 0 in af and 0 in bf[0]


@pytest.mark.parametrize("name", sorted(W.LOOKUP_CASES))
def test_reference_on_lookup_case(name):
    a, b, af, bf = W.LOOKUP_CASES[name]()
    n = len(a[0])
    assert all(len(c) == n for c in a + [c for t in b for c in t] + [af] + bf) and len(bf) == len(b)
    if name in W.LOOKUP_FAILING:
        with pytest.raises(AssertionError, match="should be 0 on the last row"):
            O.lookup_witness(a, b, af, bf, *W.challenges())
        return
    cols = W.lookup_columns(name)
    nt, nbc = len(b), len(b[0])
    occ = cols[len(a) + nt * nbc + 2 + 2 * nt:][:nt]
    assert sum(sum(c) for c in occ) == sum(1 for f in af if f)  # every enabled A row is counted once
    if name == "one_key":
        assert occ[0][2500] == n and sum(1 for x in occ[0] if x) == 1
    if name == "both_tables":
        assert (occ[0][3], occ[1][3], occ[1][2], occ[0][5]) == (2, 0, 3, 0)
    if name == "first_disabled":
        assert (occ[0][2], occ[0][5]) == (0, 3)
    if name == "high_filters":
        assert [occ[0][i] for i in (0, 1, 2, 3, 5, 8)] == [3, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("name", sorted(W.PERM_CASES))
def test_reference_on_permutation_case(name):
    a, b = W.PERM_CASES[name]()
    assert len(a) != len(b)
    cols = W.perm_columns(name)
    assert len(cols) == len(a) + len(b) + 2 and cols[-1][-1] == 1


@pytest.mark.parametrize("name", sorted(W.PERM_CASES))
def test_reference_on_padded_permutation_case(name):
    """the reference accepts the case resized with zero words to PAD_ROWS rows
    above its longest column, and its first rows are the unpadded case's"""
    a, b = W.padded_perm_case(name)
    n = len(W.PERM_CASES[name]()[0][0])
    assert all(len(c) == n + W.PAD_ROWS and c[n:] == [0] * W.PAD_ROWS for c in a + b)
    cols = W.padded_perm_columns(name)
    assert len(cols) == len(a) + len(b) + 2 and cols[-1][-1] == 1
    assert [c[:n] for c in cols] == W.perm_columns(name)


@pytest.mark.parametrize("name", W.LOOKUP_UNEVEN)
def test_reference_on_padded_lookup_case(name):
    """as above for the lookups: the padded rows are disabled (zero filters),
    so the multiplicities and the sum's end stay"""
    a, b, af, bf = W.padded_lookup_case(name)
    n = len(W.LOOKUP_CASES[name]()[0][0])
    assert all(len(c) == n + W.PAD_ROWS and c[n:] == [0] * W.PAD_ROWS for c in a + [c for t in b for c in t] + [af] + bf)
    cols = W.padded_lookup_columns(name)
    assert cols[-1][-1] == 0 and [c[:n] for c in cols] == W.lookup_columns(name)
    assert len(a) != len(b[0])  # na != nbc
    assert max(len(W.LOOKUP_CASES[k]()[1]) for k in W.LOOKUP_UNEVEN) == 2  # one of them has two tables


@pytest.mark.parametrize("n", W.PERM_SCAN_SIZES)
def test_reference_on_permutation_scan_shape(n):
    assert W.rotation_perm_columns(n)[3][-1] == 1


@pytest.mark.parametrize("n", W.LOOKUP_SCAN_SIZES)
def test_reference_on_lookup_scan_shape(n):
    assert W.rotation_lookup_columns(n)[7][-1] == 0


@pytest.mark.parametrize("log_n", [1, 5, 11])
def test_generator_model(log_n):
    n = 1 << log_n
    for seed in W.GEN_SEEDS:
        a, b = W.gen_raw_perm(seed, log_n, 2)
        mul, add = W.gen_row_map(seed, log_n)
        assert mul & 1 and sorted((mul * i + add) % n for i in range(n)) == list(range(n))
        assert sorted(zip(*a)) == sorted(zip(*b))  # the same rows in both
        assert all(0 <= v < 1 << 252 for col in a for v in col)
        assert O.perm_witness(a, b, *W.challenges())[1][-1][-1] == 1
    assert W.gen_raw_perm(W.GEN_SEEDS[0], log_n, 2) != W.gen_raw_perm(W.GEN_SEEDS[1], log_n, 2)
    if log_n > 1:
        a, b = W.gen_raw_perm(W.GEN_SEEDS[0], log_n, 1)
        assert a != b  # not the identity map
