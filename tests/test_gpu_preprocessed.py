"""Preprocessed columns on the GPU: lsp_preprocess against the existing LDE and
Merkle API, the program-capable quotient and check kernels reading a second
matrix (operand kinds 8 / 9 of k_air_prog.hpp), whole proofs against a
committed matrix (lsp_prove_preprocessed), and the calls that refuse an AIR
that reads preprocessed columns.  The reference of the quotient is the existing
kernel on the same AIR with every column in the main trace (layout "a" of
tests/preprocessed_ref.py); the reference of the check is the big-integer
evaluator and the host path; the reference of a proof is the big-integer
prover of tests/preprocessed_ref.py, byte for byte."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import check_constraints_ref as ref  # noqa: E402
import preprocessed_ref as PR  # noqa: E402
from linea_stark_prover_amd.field import GENERATOR, MODULUS, from_mont, to_mont  # noqa: E402

pytestmark = pytest.mark.gpu
R = MODULUS


def _pubs(ctx, extra):
    a, d, _ = ctx.config.seeded()
    pubi = from_mont(np.concatenate([a, d])) + list(extra)
    return pubi, to_mont(pubi)


def _seeded_matrix(h, w, seed):
    rng = np.random.default_rng(seed)
    return to_mont([int.from_bytes(rng.bytes(40), "little") % R for _ in range(h * w)]).reshape(h, w, 4)


# ---------------------------------------------------------- lsp_preprocess
@pytest.mark.parametrize("h", [2, 1 << 10])
@pytest.mark.parametrize("wp", [1, 3, 8])
def test_preprocess_is_the_lde_committed(gpu_ctx, wp, h):
    """h = 2: N = 16, every level on the host; h = 2^10: N = 2^13, device
    levels under the host's top of 1024 digests"""
    from linea_stark_prover_amd.prover import MerkleTreeMmcs
    lb = gpu_ctx.config.log_blowup
    cols = _seeded_matrix(h, wp, 100 * wp + h)
    pre = gpu_ctx.preprocess(cols)
    assert pre.width == wp and pre.tree.height == h << lb and pre.cols.shape == (h, wp, 4)
    lde = gpu_ctx.coset_lde_batch(cols, lb, to_mont([GENERATOR]))
    mmcs = MerkleTreeMmcs(gpu_ctx)
    root, tree = mmcs.commit([lde])
    assert np.array_equal(pre.commit, root)
    assert np.array_equal(pre.tree.layer(0), tree.layer(0))
    top = (h << lb).bit_length() - 1
    assert np.array_equal(pre.tree.layer(top)[0], root[0])
    for index in (0, 1, (h << lb) // 2 + 1, (h << lb) - 1):
        rows, path = mmcs.open_batch(index, pre.tree)
        assert np.array_equal(rows[0], lde[index])  # the tree owns the LDE itself
        assert mmcs.verify_batch(pre.commit, [wp], top, index, rows, path)
        assert not mmcs.verify_batch(pre.commit, [wp], top, index ^ 1, rows, path)


def test_preprocess_rejects_bad_shapes(gpu_ctx):
    from linea_stark_prover_amd import _lib as L
    for shape in ((3, 2, 4), (1, 2, 4)):
        with pytest.raises(L.LspError) as e:
            gpu_ctx.preprocess(np.zeros(shape, np.uint64))
        assert e.value.code == L.LSP_E_SIZE
    with pytest.raises(L.LspError) as e:
        gpu_ctx.preprocess(np.zeros((4, 0, 4), np.uint64))
    assert e.value.code == L.LSP_E_ARG


# ------------------------------------------------------- quotient identity
@pytest.mark.parametrize("log_h", [2, 8])
@pytest.mark.parametrize("name", sorted(PR.AIRS))
def test_quotient_values_equal_layout_a(gpu_ctx, name, log_h):
    """h = 4: a partial wave; h = 2^8: several blocks (2^10 points at four
    chunks, two 128-thread blocks for the pressure AIR's one chunk)"""
    h = 1 << log_h
    wp, w, _ = PR.AIRS[name]
    fixed, main, extra = PR.build_rows(name, h)
    _, pub = _pubs(gpu_ctx, extra)
    lde = gpu_ctx.coset_lde_batch(PR.to_matrix(PR.joined(fixed, main)), gpu_ctx.config.log_blowup,
                                  to_mont([GENERATOR]))
    alpha = to_mont([0x1234567 * 0x89abcdef + 5])
    exp = gpu_ctx.quotient_values(lde, h, PR.build_air(name, "a"), pub, alpha)
    got = gpu_ctx.quotient_values(np.ascontiguousarray(lde[:, wp:]), h, PR.build_air(name, "b"), pub, alpha,
                                  prep_lde=np.ascontiguousarray(lde[:, :wp]))
    assert got.shape[0] == h << PR.LOG_Q[name] and got.tobytes() == exp.tobytes()
    # the values are a quotient's: the trace satisfies the AIR, so they are not all zero
    # and differ once a fixed column is another one
    assert got.any()
    other = np.ascontiguousarray(lde[:, :wp][::-1])
    bad = gpu_ctx.quotient_values(np.ascontiguousarray(lde[:, wp:]), h, PR.build_air(name, "b"), pub, alpha,
                                  prep_lde=other)
    assert bad.tobytes() != exp.tobytes()


# ------------------------------------------------------------------ check
@pytest.mark.parametrize("log_h", [2, 9])
@pytest.mark.parametrize("name", sorted(PR.AIRS))
def test_device_check_equals_host_and_evaluator(gpu_ctx, name, log_h):
    from linea_stark_prover_amd.prover import Context, StarkConfig
    h = 1 << log_h
    wp, w, _ = PR.AIRS[name]
    air = PR.build_air(name, "b")
    fixed, main, extra = PR.build_rows(name, h)
    pubi, pub = _pubs(gpu_ctx, extra)
    host = Context(StarkConfig(), device=-1)
    try:
        cases = [(None, 0, 0), ("main", h - 1, w - 1), ("main", h // 2, 0), ("fixed", h // 2, wp - 1),
                 ("fixed", 0, 0), ("fixed", h - 1, wp - 1)]
        bad = 0
        for where, r_, c in cases:
            ff, mm = [list(x) for x in fixed], [list(x) for x in main]
            if where:
                t = mm if where == "main" else ff
                t[r_][c] = (t[r_][c] + 1) % R
            exp = PR.report(air, mm, pubi, 16, ff)
            # (a fault in the last row's fixed cell may go unread: the transition selector is off there)
            assert exp["ok"] if where is None else True
            bad += not exp["ok"]
            dev = gpu_ctx.check_constraints(PR.to_matrix(mm), air, pub, preprocessed=PR.to_matrix(ff))
            cpu = host.check_constraints(PR.to_matrix(mm), air, pub, preprocessed=PR.to_matrix(ff))
            assert ref.as_dict(dev) == exp == ref.as_dict(cpu)
        assert bad >= 3
    finally:
        host.close()


# --------------------------------------------------------------- refusals
def test_calls_without_a_preprocessed_matrix_refuse(gpu_ctx):
    """refused on the host before any launch: the prove calls, the group prove,
    the plain quotient and check, a matrix narrower than the AIR reads"""
    from linea_stark_prover_amd import _lib as L
    from linea_stark_prover_amd.prover import ProverGroup
    air = PR.build_air("gated", "b")
    fixed, main, extra = PR.build_rows("gated", 8)
    _, pub = _pubs(gpu_ctx, extra)
    trace = PR.to_matrix(main)
    lde = gpu_ctx.coset_lde_batch(PR.to_matrix(PR.joined(fixed, main)), gpu_ctx.config.log_blowup,
                                  to_mont([GENERATOR]))
    alpha = to_mont([7])
    grp = ProverGroup([gpu_ctx])
    calls = [lambda: gpu_ctx.prove(trace, air, pub),
             lambda: grp.prove(trace, air, pub),
             lambda: gpu_ctx.check_constraints(trace, air, pub),
             lambda: gpu_ctx.quotient_values(np.ascontiguousarray(lde[:, 2:]), 8, air, pub, alpha),
             lambda: gpu_ctx.quotient_values(np.ascontiguousarray(lde[:, 2:]), 8, air, pub, alpha,
                                             prep_lde=np.ascontiguousarray(lde[:, :1])),
             lambda: gpu_ctx.check_constraints(trace, air, pub, preprocessed=PR.to_matrix(fixed)[:, :1])]
    try:
        for f in calls:
            with pytest.raises(L.LspError) as e:
                f()
            assert e.value.code == L.LSP_E_ARG and "preprocessed columns" in str(e.value)
    finally:
        grp.close()
    # and the context is as usable as before
    assert gpu_ctx.check_constraints(trace, air, pub, preprocessed=PR.to_matrix(fixed)).ok


# ------------------------------------------------------------ whole proofs
def _setup():
    from oracle import pyoracle as O
    return O.setup_from_seed()


@pytest.fixture(scope="module")
def reference():
    """(name, h) -> (the big-integer prover's proof, its log, fixed, main, pub ints), made once"""
    cache = {}

    def get(name, h, x0=5):
        if (name, h, x0) not in cache:
            s = _setup()
            fixed, main, extra = PR.build_rows(name, h, x0) if name != "pressure" else PR.build_rows(name, h)
            pubi = [s.alpha, s.delta] + extra
            proof, log = PR.prove(PR.build_air(name, "b"), main, fixed, pubi, s.perm)
            cache[(name, h, x0)] = (proof, log, fixed, main, pubi)
        return cache[(name, h, x0)]
    return get


@pytest.mark.parametrize("early", ["0", "1"])
@pytest.mark.parametrize("name,h", [("keyed", 2), ("gated", 4), ("wide", 4), ("gated", 32), ("pressure", 32)])
def test_proofs_are_the_reference_provers(gpu_ctx, reference, monkeypatch, name, h, early):
    """byte for byte, with wp > w (gated), w > wp (wide) and the 128-thread block form (pressure)"""
    monkeypatch.setenv("LSP_QUOTIENT_EARLY", early)
    exp, log, fixed, main, pubi = reference(name, h)
    air, pub = PR.build_air(name, "b"), to_mont(pubi)
    pre = gpu_ctx.preprocess(PR.to_matrix(fixed))
    assert from_mont(pre.commit)[0] == log["prep_root"]
    got = gpu_ctx.prove(PR.to_matrix(main), air, pub, preprocessed=pre)
    assert got[:8] == b"LSPPRF03" and got == exp
    assert gpu_ctx.verify(got, air, pub, preprocessed=pre)
    assert gpu_ctx.verify(got, air, pub, preprocessed=(pre.commit, pre.width))
    assert not gpu_ctx.verify(got, air, pub, preprocessed=(pre.commit, pre.width + 1))


@pytest.mark.parametrize("log_h", [10, 13])
def test_larger_proofs_verify(gpu_ctx, log_h):
    """device tree levels under the host's top, the FRI host / device boundary
    crossed; one AIR mixes a built-in permutation config with a type-4 program"""
    from linea_stark_prover_amd import prover as P
    from linea_stark_prover_amd.air import LineaAIR, permutation_air
    h = 1 << log_h
    a, d, _ = gpu_ctx.config.seeded()
    fixed, main, extra = PR.build_rows("keyed", h)
    pubi, pub = _pubs(gpu_ctx, extra)
    prog = PR.build_air("keyed", "b").configs[0]
    prog.shift(4)
    air = LineaAIR([permutation_air(1).configs[0], prog])
    trace = np.concatenate([P.gen_permutation_trace(log_h, 1, a, d), PR.to_matrix(main)], axis=1)
    pre = gpu_ctx.preprocess(PR.to_matrix(fixed))
    assert gpu_ctx.check_constraints(trace, air, pub, preprocessed=pre).ok
    proof = gpu_ctx.prove(trace, air, pub, preprocessed=pre, check=True)
    assert gpu_ctx.verify(proof, air, pub, preprocessed=pre)
    # zeta replayed from the proof's roots; the opened preprocessed values are the
    # interpolation of the tree's low coset (its matrix is the LDE: the commit test) there
    from oracle import pyoracle as O
    pf = PR.parse(proof)
    assert (pf["log_h"], pf["w"], pf["wp"]) == (log_h, 5, 1) and pf["trace_root"] != pf["quotient_root"]
    ch = O.HashChallenger(_setup().perm)
    ch.observe(log_h)
    ch.observe(pf["trace_root"])
    ch.observe(from_mont(pre.commit)[0])
    ch.observe_slice(pubi)
    ch.sample()  # alpha
    ch.observe(pf["quotient_root"])
    zeta = ch.sample()
    low = gpu_ctx.coset_lde_batch(PR.to_matrix(fixed), gpu_ctx.config.log_blowup, to_mont([GENERATOR]))[:h]
    low = [[x] for x in from_mont(low.reshape(-1, 4))]
    assert pf["prep_local"] == O.interpolate_coset(low, O.GENERATOR, zeta)
    assert pf["prep_next"] == O.interpolate_coset(low, O.GENERATOR, zeta * O.two_adic_generator(log_h) % R)
    # another commitment, another public value, a flipped opened preprocessed value
    other = gpu_ctx.preprocess(PR.to_matrix([[x + 1 for x in r] for r in fixed]))
    assert not gpu_ctx.verify(proof, air, pub, preprocessed=other)
    bad = list(pubi)
    bad[2] = (bad[2] + 1) % R
    assert not gpu_ctx.verify(proof, air, to_mont(bad), preprocessed=pre)
    flipped = bytearray(proof)
    flipped[8 + 28 + 32 * (2 + 2 * 5 + 1) + 3] ^= 0x10  # prep@zeta[0]: after the header, two roots, 2w + q values
    assert not gpu_ctx.verify(bytes(flipped), air, pub, preprocessed=pre)
    # the gated AIR alone at this height: four chunks, wp > w
    f2, m2, e2 = PR.build_rows("gated", h)
    _, pub2 = _pubs(gpu_ctx, e2)
    pre2 = gpu_ctx.preprocess(PR.to_matrix(f2))
    air2 = PR.build_air("gated", "b")
    proof2 = gpu_ctx.prove(PR.to_matrix(m2), air2, pub2, preprocessed=pre2)
    assert gpu_ctx.verify(proof2, air2, pub2, preprocessed=pre2)
    assert not gpu_ctx.verify(proof2, air2, pub2, preprocessed=(pre.commit, 2))  # another matrix's root


def test_one_tree_serves_many_proofs(gpu_ctx, reference):
    """two traces against one tree, an ordinary proof of another shape in
    between on the same context, then the first proof again, byte for byte:
    a tree left in a pool buffer would not survive this"""
    from linea_stark_prover_amd import prover as P
    from linea_stark_prover_amd.air import permutation_air
    exp1, log, fixed, main1, pubi1 = reference("gated", 32)
    exp2, _, fixed2, main2, pubi2 = reference("gated", 32, x0=11)
    assert fixed == fixed2 and main1 != main2 and exp1 != exp2
    air = PR.build_air("gated", "b")
    pre = gpu_ctx.preprocess(PR.to_matrix(fixed))
    assert gpu_ctx.prove(PR.to_matrix(main1), air, to_mont(pubi1), preprocessed=pre) == exp1
    assert gpu_ctx.prove(PR.to_matrix(main2), air, to_mont(pubi2), preprocessed=pre) == exp2
    a, d, _ = gpu_ctx.config.seeded()
    for log_n, ncols in ((5, 2), (12, 3)):  # the same and a larger LDE height, other widths
        tr = P.gen_permutation_trace(log_n, ncols, a, d)
        pub = np.concatenate([a, d])
        assert gpu_ctx.verify(gpu_ctx.prove(tr, permutation_air(ncols), pub), permutation_air(ncols), pub)
    assert gpu_ctx.prove(PR.to_matrix(main1), air, to_mont(pubi1), preprocessed=pre) == exp1
    assert from_mont(pre.commit)[0] == log["prep_root"]
    assert np.array_equal(pre.tree.layer(8)[0], pre.commit[0])


def test_unfit_trees_are_refused(gpu_ctx):
    from linea_stark_prover_amd import _lib as L
    from linea_stark_prover_amd.prover import MerkleTreeMmcs
    lb = gpu_ctx.config.log_blowup
    fixed, main, extra = PR.build_rows("gated", 8)
    _, pub = _pubs(gpu_ctx, extra)
    air, trace = PR.build_air("gated", "b"), PR.to_matrix(main)
    lde = gpu_ctx.coset_lde_batch(PR.to_matrix(fixed), lb, to_mont([GENERATOR]))
    mmcs = MerkleTreeMmcs(gpu_ctx)
    short = gpu_ctx.preprocess(PR.to_matrix(fixed[:4]))              # another height
    _, two = mmcs.commit([lde, lde])                                  # two matrices
    _, narrow = mmcs.commit([np.ascontiguousarray(lde[:, :1])])       # fewer columns than the AIR reads
    for tree in (short, two, narrow):
        with pytest.raises(L.LspError) as e:
            gpu_ctx.prove(trace, air, pub, preprocessed=tree)
        assert e.value.code == L.LSP_E_ARG
    # a tree of another context is refused, on the same device too: its uploads ran on that
    # context's stream, and this call holds only its own context's mutex
    from linea_stark_prover_amd.prover import Context, StarkConfig
    with Context(StarkConfig()) as other:
        foreign = other.preprocess(PR.to_matrix(fixed))
        try:
            gpu_ctx.prove(trace, air, pub, preprocessed=foreign)
            refused = None
        except L.LspError as err:
            refused = (err.code, str(err))  # (the exception's traceback would keep the tree alive)
        assert refused and refused[0] == L.LSP_E_ARG and "another context" in refused[1]
        assert other.verify(other.prove(trace, air, pub, preprocessed=foreign), air, pub, preprocessed=foreign)
        # a tree is freed before its context
        L.lib().lsp_tree_free(foreign.tree.handle)
        foreign.tree.handle = None
    # a tree from lsp_merkle_commit over a caller-made LDE qualifies
    root, own = mmcs.commit([lde])
    proof = gpu_ctx.prove(trace, air, pub, preprocessed=own)
    assert gpu_ctx.verify(proof, air, pub, preprocessed=(root, 2))
    assert proof == gpu_ctx.prove(trace, air, pub, preprocessed=gpu_ctx.preprocess(PR.to_matrix(fixed)))


# ------------------------------------- k_reduce_matrix's edges inside a proof
# The kernel that adds the preprocessed matrix's terms to the FRI input loads a
# row in chunks of three columns (RR_CHUNK), one chunk ahead, and keeps the wp
# alpha powers in dynamic LDS behind the 3 KiB reduction table: 36 bytes a
# column, over 48 KiB from wp = 1281 (asked for by attribute), refused past the
# device's LDS per workgroup.  PR.keyed_sum(wp) reads every one of wp columns
# in one slot, so only this kernel's limits are in play.
QTAB_BYTES, APW_BYTES = 3 * 64 * 16, 36


@pytest.fixture(scope="module")
def keyed_sum_reference():
    """(wp, h) -> (the big-integer prover's proof, its log, fixed, main, pub ints), made once"""
    cache = {}

    def get(wp, h):
        if (wp, h) not in cache:
            s = _setup()
            fixed, main, extra = PR.keyed_sum_rows(wp, h)
            pubi = [s.alpha, s.delta] + extra
            proof, log = PR.prove(PR.keyed_sum(wp), main, fixed, pubi, s.perm)
            cache[(wp, h)] = (proof, log, fixed, main, pubi)
        return cache[(wp, h)]
    return get


@pytest.mark.parametrize("wp,h", [(2, 4), (3, 4), (4, 4), (5, 4), (6, 4), (7, 4), (7, 64)])
def test_chunk_boundaries_of_the_prep_reduction(gpu_ctx, keyed_sum_reference, wp, h):
    """widths below, at and above one and two chunks of three, byte for byte;
    h = 64: 512 LDE rows, two blocks"""
    exp, log, fixed, main, pubi = keyed_sum_reference(wp, h)
    air, pub = PR.keyed_sum(wp), to_mont(pubi)
    pre = gpu_ctx.preprocess(PR.to_matrix(fixed))
    assert pre.width == wp and from_mont(pre.commit)[0] == log["prep_root"]
    got = gpu_ctx.prove(PR.to_matrix(main), air, pub, preprocessed=pre)
    assert got == exp
    assert gpu_ctx.verify(got, air, pub, preprocessed=pre)


def test_prep_reduction_over_48_kib_of_lds(gpu_ctx, keyed_sum_reference):
    wp, h = 1300, 2
    assert QTAB_BYTES + APW_BYTES * wp > 48 * 1024 >= QTAB_BYTES + APW_BYTES * 1280
    exp, log, fixed, main, pubi = keyed_sum_reference(wp, h)
    air, pub = PR.keyed_sum(wp), to_mont(pubi)
    pre = gpu_ctx.preprocess(PR.to_matrix(fixed))
    got = gpu_ctx.prove(PR.to_matrix(main), air, pub, preprocessed=pre)
    assert got == exp
    assert gpu_ctx.verify(got, air, pub, preprocessed=pre)
    for col in (0, wp - 1):  # a flipped opened preprocessed value, the first and the last column
        flipped = bytearray(got)
        flipped[log["marks"]["prep_local"] + 32 * col + 3] ^= 0x10
        assert not gpu_ctx.verify(bytes(flipped), air, pub, preprocessed=pre)


def _lds_per_workgroup():
    """hipDeviceProp_t::sharedMemPerBlock of device 0 (what the context's
    hipDeviceAttributeMaxSharedMemoryPerBlock query answers), from the runtime
    the library has loaded"""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    prop = ctypes.create_string_buffer(8192)
    assert hip.hipGetDevicePropertiesR0600(prop, 0) == 0
    return int.from_bytes(prop.raw[296:304], "little")  # after name[256], uuid, luid, the mask, totalGlobalMem


def test_refusal_boundary_of_the_prep_reduction(gpu_ctx):
    """the widest matrix whose alpha powers the LDS holds proves and verifies, one
    column more is LSP_E_ARG and leaves the context usable"""
    from linea_stark_prover_amd import _lib as L
    from linea_stark_prover_amd import prover as P
    from linea_stark_prover_amd.air import permutation_air
    lds = _lds_per_workgroup()
    assert lds in (64 * 1024, 160 * 1024), lds
    wp_max = (lds - QTAB_BYTES) // APW_BYTES
    if lds == 160 * 1024:  # gfx950
        assert wp_max == 4465
    h = 2
    a, d, _ = gpu_ctx.config.seeded()
    for wp in (wp_max + 1, wp_max):
        fixed, main, extra = PR.keyed_sum_rows(wp, h)
        pubi, pub = _pubs(gpu_ctx, extra)
        air = PR.keyed_sum(wp)
        assert PR.report(air, main, pubi, 4, fixed)["ok"]
        pre = gpu_ctx.preprocess(PR.to_matrix(fixed))
        if wp > wp_max:
            with pytest.raises(L.LspError, match="wider than the reduce kernel's LDS holds") as e:
                gpu_ctx.prove(PR.to_matrix(main), air, pub, preprocessed=pre)
            assert e.value.code == L.LSP_E_ARG
            # the context proves an ordinary trace afterwards
            tr = P.gen_permutation_trace(5, 2, a, d)
            pub2 = np.concatenate([a, d])
            assert gpu_ctx.verify(gpu_ctx.prove(tr, permutation_air(2), pub2), permutation_air(2), pub2)
        else:
            proof = gpu_ctx.prove(PR.to_matrix(main), air, pub, preprocessed=pre)
            assert gpu_ctx.verify(proof, air, pub, preprocessed=pre)
            assert not gpu_ctx.verify(proof, air, pub, preprocessed=(pre.commit, wp + 1))
