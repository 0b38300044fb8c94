"""Zero denominators: the batch inverse maps 0 to 0 and leaves every other
element's inverse as it is (csrc/kernels.hpp), and the callers that cannot
use a zero denominator refuse it instead of returning a finished-looking
result: the witness generators (the reference panics in Field::inverse) and
the open stage's entry points (a point on the coset).

Checker: Python big ints / pyoracle.  Bit-exact.

The batch inverse's shape: workgroups of 256 threads own 4096 elements,
thread t the 16 elements t + 256 j of its workgroup; up to 4096 elements one
base kernel, above that one up/down level per factor of 4096.
"""
import functools
import os
import sys

import numpy as np
import pytest

from oracle import pyoracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import inverse_zero_cases as Z  # noqa: E402

pytestmark = pytest.mark.gpu

P = O.P
THREADS, CHUNK, WG = 256, 16, 4096
BLOCK = 2999  # values per tile: a prime, so a tile never lines up with a thread's stride


def mont(vals):
    from linea_stark_prover_amd.field import to_mont
    return to_mont(list(vals))


def ints(a):
    from linea_stark_prover_amd.field import from_mont
    return from_mont(a.reshape(-1, 4))


# ------------------------------------------------------------ batch inverse
@functools.lru_cache(maxsize=None)
def block():
    """BLOCK non-zero values and their inverses (pow(v, P - 2, P), once), Montgomery form"""
    edges = [1, P - 1, P - 2, 1 << 252, (1 << 256) % P, 2, (P - 1) // 2, (P + 1) // 2, 0xFFFFFFFF]
    rng = O.SplitMix64(0x5A45524F)
    vals = edges + [rng.sample_fr() or 1 for _ in range(BLOCK - len(edges))]
    return mont(vals), mont([pow(v, P - 2, P) for v in vals])


def thread_chunk(n, g, t):
    """the indices thread t of workgroup g owns: g 4096 + t + 256 j below n"""
    return [i for i in range(g * WG + t, min(n, (g + 1) * WG), THREADS)]


def a_thread(n):
    """(workgroup, thread) of a chunk away from both ends: thread 5 of the
    second workgroup where that has one, else of the first"""
    return (1 if n > WG + 5 else 0), 5


def placements(n):
    """name -> zero positions, for every placement that fits n"""
    g, t = a_thread(n)
    chunk = thread_chunk(n, g, t)
    out = {"first": [0], "last": [n - 1], "every_second": range(0, n, 2), "all": range(n)}
    if n >= 2:
        out["both_ends"] = [0, n - 1]
    if len(chunk) >= 2:  # the ends of one thread's strided chunk, and the whole of it
        out["chunk_first"] = chunk[:1]
        out["chunk_last"] = chunk[-1:]  # k_bi_down rebuilds the chunk's product from this element
        out["whole_chunk"] = chunk
    if n >= WG:  # a workgroup whose every input is zero: its product goes up a level
        gz = 1 if n >= 2 * WG else 0
        out["whole_workgroup"] = range(gz * WG, (gz + 1) * WG)
    if n > WG and n % WG == 1:
        out["lone_tail"] = [n - 1]  # the partial last workgroup's only element
    if n > WG and n % WG > 1:  # the partial last workgroup whole (fewer than 16 elements per thread)
        out["whole_tail"] = range(n - n % WG, n)
    return out


BASE = [1, 2, 255, 256, 257, 4095, 4096]
ONE_LEVEL = [4097, 4096 + 255, 4096 + 257, 8191, 8192, 3 * 4096 + 1]
CASES = [(n, name) for n in BASE + ONE_LEVEL for name in placements(n)]


def check_batch_inverse(ctx, n, zeros):
    vals, invs = block()
    tile = np.arange(n) % BLOCK
    x, exp = vals[tile], invs[tile]
    z = np.fromiter(zeros, dtype=np.int64)
    x[z] = 0
    exp[z] = 0
    got = ctx.batch_inverse(x)
    if not np.array_equal(got, exp):
        bad = np.flatnonzero((got != exp).any(axis=1))
        nz = np.setdiff1d(bad, z)
        pytest.fail(f"n = {n}: {bad.size} of {n} outputs wrong ({nz.size} of them at non-zero inputs), "
                    f"the first at {bad[0]}")


def test_block_is_what_it_says():
    vals, invs = block()
    v, i = ints(vals), ints(invs)
    assert len(v) == BLOCK and all(a and a * b % P == 1 for a, b in zip(v, i))
    assert {1, P - 1, P - 2, 1 << 252, (1 << 256) % P} <= set(v)


@pytest.mark.parametrize("n,where", CASES, ids=[f"{n}-{w}" for n, w in CASES])
def test_batch_inverse_with_zeros(gpu_ctx, n, where):
    check_batch_inverse(gpu_ctx, n, placements(n)[where])


def test_batch_inverse_with_zeros_two_levels(gpu_ctx):
    """2^24 + 1 elements (4097 workgroups: two up/down levels above the base),
    one run with the sparse placements together: both ends (the last is the
    partial workgroup's only element), a thread chunk's first and last element
    in two more workgroups, a whole thread chunk, a whole workgroup, and three
    adjacent workgroups of zeros (neighbours one level up)"""
    n = (1 << 24) + 1
    pl = placements(n)
    zeros = set(pl["both_ends"]) | set(pl["whole_chunk"]) | set(pl["whole_workgroup"])
    zeros |= {thread_chunk(n, 7, 255)[0], thread_chunk(n, 4095, 0)[-1]}
    zeros |= set(range(2000 * WG, 2000 * WG + 3 * WG))  # three adjacent workgroups of zeros
    check_batch_inverse(gpu_ctx, n, sorted(zeros))


def test_batch_inverse_zero_does_not_stick(gpu_ctx):
    """the scratch products of a call with zeros are not read by the next call"""
    check_batch_inverse(gpu_ctx, 3 * WG + 1, range(0, 3 * WG + 1))
    check_batch_inverse(gpu_ctx, 3 * WG + 1, [])


# ------------------------------------------------------------------ witness
def _mont_cols(cols):
    return [mont(c) for c in cols]


def _raw_trace(ctx):
    from linea_stark_prover_amd.trace import RawTrace
    al, de = Z.challenges()
    return RawTrace(ctx, [mont([al]), mont([de])])


def _lookup_trace(case):
    from linea_stark_prover_amd.trace import RawLookupTrace
    a, b, af, bf = case
    return RawLookupTrace(_mont_cols(a), [_mont_cols(t) for t in b], mont(af), [mont(f) for f in bf])


def _perm_trace(case):
    from linea_stark_prover_amd.trace import RawPermutationTrace
    return RawPermutationTrace(_mont_cols(case[0]), _mont_cols(case[1]))


@functools.lru_cache(maxsize=None)
def _good_lookup_columns(n):
    good, _ = Z.lookup_case(n, Z.LOOKUP_SPOTS[0])  # `good` is the same for every spot
    return np.stack(_mont_cols(O.lookup_witness(*good, *Z.challenges())[1]), axis=1)


def _refused(push):
    from linea_stark_prover_amd import _lib
    with pytest.raises(_lib.LspError) as e:
        push()
    assert e.value.code == _lib.LSP_E_STATE, e.value
    assert "invert zero" in str(e.value), e.value
    assert "last row" not in str(e.value), e.value


@pytest.mark.parametrize("spot", Z.LOOKUP_SPOTS)
@pytest.mark.parametrize("n", Z.LOOKUP_SIZES)
def test_lookup_witness_refuses_zero_denominator(gpu_ctx, n, spot):
    """one cell with comb + delta = 0, in an enabled or a disabled row of the
    table or of A: the reference inverts every row and panics; every inverse
    column zeroed would close the LogUp sum and pass for a witness"""
    good, bad = Z.lookup_case(n, spot)
    rt = _raw_trace(gpu_ctx)
    try:
        _refused(lambda: rt.push_traces([], [_lookup_trace(bad)]))
        rt.push_traces([], [_lookup_trace(good)])  # the same RawTrace and context go on working
        assert np.array_equal(rt.get_trace(host=True), _good_lookup_columns(n))
    finally:
        rt.close()


@pytest.mark.parametrize("n", Z.PERM_SIZES)
def test_permutation_witness_refuses_zero_denominator(gpu_ctx, n):
    """a valid permutation with one B row of comb + delta = 0: a zero
    denominator, not a check column that fails to close"""
    good, bad = Z.perm_case(n)
    rt = _raw_trace(gpu_ctx)
    try:
        _refused(lambda: rt.push_traces([_perm_trace(bad)], []))
        rt.push_traces([_perm_trace(good)], [])
        exp = np.stack(_mont_cols(O.perm_witness(*good, *Z.challenges())[1]), axis=1)
        assert np.array_equal(rt.get_trace(host=True), exp)
    finally:
        rt.close()


# --------------------------------------------------------------- open stage
SHIFT = O.GENERATOR
LOGS = [0, 1, 3, 7]


def _on_coset(log_n):
    """shift w_N^k for k in {0, 1, N - 1}"""
    N, g = 1 << log_n, O.two_adic_generator(log_n)
    return [SHIFT * pow(g, k, P) % P for k in sorted({0, 1 % N, N - 1})]


def _near_misses(log_n):
    """on the doubled coset but not on the coset; zero"""
    return [SHIFT * O.two_adic_generator(log_n + 1) % P, 0]


def _matrix(log_n, w=3):
    rng = O.SplitMix64(40 + log_n)
    return [[rng.sample_fr() for _ in range(w)] for _ in range(1 << log_n)]


def _arg_error(call):
    from linea_stark_prover_amd import _lib
    with pytest.raises(_lib.LspError) as e:
        call()
    assert e.value.code == _lib.LSP_E_ARG, e.value


@pytest.mark.parametrize("log_n", LOGS)
def test_inverse_denominators_refuse_a_point_on_the_coset(gpu_ctx, log_n):
    sh = mont([SHIFT])
    off = _near_misses(log_n)
    for z in _on_coset(log_n):
        _arg_error(lambda: gpu_ctx.inverse_denominators(mont([z]), log_n, sh))
        for pts in ([z] + off, [off[0], z, off[1]], off + [z]):  # one bad point among three
            _arg_error(lambda: gpu_ctx.inverse_denominators(mont(pts), log_n, sh))
    _arg_error(lambda: gpu_ctx.inverse_denominators(mont(off), log_n, mont([0])))
    # the near misses are points like any other
    got = gpu_ctx.inverse_denominators(mont(off), log_n, sh)
    assert [ints(got[p]) for p in range(len(off))] == O.inverse_denominators(log_n, SHIFT, off)


@pytest.mark.parametrize("log_n", LOGS)
def test_interpolate_coset_refuses_a_point_on_the_coset(gpu_ctx, log_n):
    """there the interpolated value is the matrix row itself; the barycentric
    formula has no value, p3 panics, and zeros must not come back"""
    h, sh = 1 << log_n, mont([SHIFT])
    rows = _matrix(log_n)
    mat = mont([x for r in rows for x in r]).reshape(h, 3, 4)
    for z in _on_coset(log_n):
        _arg_error(lambda: gpu_ctx.interpolate_coset(mat, h, sh, mont([z])))
    _arg_error(lambda: gpu_ctx.interpolate_coset(mat, h, mont([0]), mont([5])))
    for z in _near_misses(log_n):
        assert ints(gpu_ctx.interpolate_coset(mat, h, sh, mont([z]))) == O.interpolate_coset(rows, SHIFT, z), z
