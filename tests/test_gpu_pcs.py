"""TwoAdicFriPcs over batches of unequal heights on the GPU (DESIGN.md section 3,
U15): lsp_pcs_commit / lsp_pcs_open against the big-integer reference of
tests/pcs_ref.py on the shapes of tests/pcs_cases.py -- commitments, opened
values and proofs byte for byte -- the existing prover's proof field by field
on its own shape, the lane forms of the fused fold-and-hash kernel (one
child process per setting; at true widths against the 4-lane form and the host
verifier), and the commit phase's host paths under roll-ins.  Everything is
bit-exact.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import pcs_cases as C  # noqa: E402
import pcs_ref as R  # noqa: E402
from linea_stark_prover_amd.field import from_mont, to_mont  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
P = O.P


def to_arrays(mats):
    return [to_mont([x for row in m for x in row]).reshape(len(m), len(m[0]), 4) for m in mats]


def gpu_open(ctx, name, device=False):
    """the case's transcript on the product: commit every batch, observe the
    roots, sample z, open.  Returns (roots, opened values, proof bytes, trees,
    the challenger as open left it)."""
    from linea_stark_prover_amd.prover import HashChallenger, TwoAdicFriPcs
    pcs, roots, trees = TwoAdicFriPcs(ctx), [], []
    for ms, b in zip(C.matrices(name), C.CASES[name][0]):
        arrs, shifts = to_arrays(ms), to_mont([s for _, _, s, _ in b])
        if all(s == 1 for _, _, s, _ in b):
            shifts = None  # the NULL argument
        if device:
            dev = [ctx.dev_alloc(a.nbytes) for a in arrs]
            for p, a in zip(dev, arrs):
                ctx.h2d(p, a)
            try:
                root, tree = pcs.commit(dev, shifts, dims=[a.shape[:2] for a in arrs])
            finally:
                for p in dev:
                    ctx.dev_free(p)
        else:
            root, tree = pcs.commit(arrs, shifts)
        roots.append(root)
        trees.append(tree)
    ch = HashChallenger(ctx)
    ch.observe(np.concatenate(roots))
    z = from_mont(ch.sample())[0]
    rounds = [(t, [to_mont(zs) for zs in pts]) for t, pts in zip(trees, C.points_of(name, z))]
    opened, wire = pcs.open(rounds, ch)
    return roots, opened, wire, trees, ch


_ctxs = {}


def ctx_for(name):
    """one context per distinct configuration among the cases"""
    from linea_stark_prover_amd.prover import Context
    key = tuple(sorted(C.CASES[name][1].items()))
    if key not in _ctxs:
        _ctxs[key] = Context(C.stark_config(name))
    return _ctxs[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts(product_lib):
    yield
    for ctx in _ctxs.values():
        ctx.close()
    _ctxs.clear()


def check_against_reference(ctx, name, device=False):
    ref, fri = C.reference(name), C.fri_of(name)
    roots, opened, wire, trees, ch = gpu_open(ctx, name, device)
    assert [from_mont(r)[0] for r in roots] == [c.root for c in ref.coms]
    got = [[[from_mont(pt) for pt in m] for m in b] for b in opened]
    assert got == ref.proof.ys
    assert wire == ref.wire
    # the challenger is left where the reference's is
    want = O.HashChallenger(C.pp(), mont_bits=fri.sample_bits_montgomery)
    want.input_buffer, want.output_buffer = list(ref.state[0]), list(ref.state[1])
    assert from_mont(ch.sample())[0] == want.sample()
    return trees


@pytest.mark.parametrize("name", [n for n in C.CASES if n != "ladder_2e10"])
def test_proofs_equal_the_references(product_lib, name):
    check_against_reference(ctx_for(name), name)


def test_device_input_pointers(product_lib):
    check_against_reference(ctx_for("classes"), "classes", device=True)
    check_against_reference(ctx_for("shifts"), "shifts", device=True)


def test_commit_returns_an_ordinary_tree(product_lib):
    """lsp_tree_dims reports the LDE heights; lsp_merkle_open and lsp_merkle_layer work on the tree"""
    import ctypes
    from linea_stark_prover_amd import _lib
    from linea_stark_prover_amd.prover import MerkleTreeMmcs
    name = "gaps"
    ctx, ref = ctx_for(name), C.reference(name)
    tree = gpu_open(ctx, name)[3][0]
    hs, ws, n = (ctypes.c_size_t * 4)(), (ctypes.c_size_t * 4)(), ctypes.c_size_t()
    assert _lib.lib().lsp_tree_dims(tree.handle, hs, ws, 4, ctypes.byref(n)) == 0
    want = ref.coms[0]
    assert n.value == 2 and list(hs[:2]) == [len(m) for m in want.ldes] and list(ws[:2]) == [2, 3]
    for level, layer in enumerate(want.tree.layers):
        assert from_mont(tree.layer(level)) == layer
    for index in (0, 77, len(want.ldes[0]) - 1):
        rows, path = MerkleTreeMmcs(ctx).open_batch(index, tree)
        w_rows, w_path = R.MM.open(want.tree, index)
        assert [from_mont(r) for r in rows] == w_rows and from_mont(path) == w_path


# ----------------------------------------- cross-check with the prover
def test_open_equals_the_provers_own_open(gpu_ctx):
    """the 3x3 permutation AIR at h = 64: the challenger replayed to where
    lsp_prove opens, the chunks from Context.quotient_values; TwoAdicFriPcs.open
    then gives lsp_proof_get_view's fields of Context.prove's proof"""
    from linea_stark_prover_amd.air import permutation_air
    from linea_stark_prover_amd.proof import Proof
    from linea_stark_prover_amd.prover import HashChallenger, TwoAdicFriPcs, gen_permutation_trace
    ctx, log_h = gpu_ctx, 6
    h, lb = 1 << log_h, ctx.config.log_blowup
    a, d, _ = ctx.config.seeded()
    trace, air, pub = gen_permutation_trace(log_h, 3, a, d), permutation_air(3), np.concatenate([a, d])
    want = Proof.from_bytes(ctx.prove(trace, air, pub))

    pcs, ch = TwoAdicFriPcs(ctx), HashChallenger(ctx)
    troot, ttree = pcs.commit([trace])
    assert np.array_equal(troot, want.commitments.trace)
    ch.observe(to_mont([log_h]))
    ch.observe(troot)
    ch.observe(pub)
    alpha = ch.sample()
    lde = ctx.coset_lde_batch(trace, lb, to_mont([O.GENERATOR]))
    qv = ctx.quotient_values(lde, h, air, pub, alpha)
    q = qv.shape[0] // h
    chunks = [np.ascontiguousarray(qv.reshape(h, q, 4)[:, j:j + 1]) for j in range(q)]
    gq = O.two_adic_generator(log_h + O.log2_strict(q))
    qroot, qtree = pcs.commit(chunks, to_mont([O.GENERATOR * pow(gq, j, P) % P for j in range(q)]))
    assert np.array_equal(qroot, want.commitments.quotient_chunks)
    ch.observe(qroot)
    zeta = from_mont(ch.sample())[0]
    pts = to_mont([zeta, zeta * O.two_adic_generator(log_h) % P])
    opened, wire = pcs.open([(ttree, [pts]), (qtree, [pts[:1]] * q)], ch)

    ov, fp = want.opened_values, want.opening_proof
    assert np.array_equal(opened[0][0][0], ov.trace_local) and np.array_equal(opened[0][0][1], ov.trace_next)
    assert all(np.array_equal(opened[1][j][0], ov.quotient_chunks[j]) for j in range(q))
    got = R.parse(wire)
    assert got.roots == from_mont(fp.commit_phase_commits)
    assert got.final_poly == from_mont(fp.final_poly) and [got.pow_witness] == from_mont(fp.pow_witness)
    assert len(got.queries) == len(fp.query_proofs) == ctx.config.num_queries
    for (inputs, steps), qp in zip(got.queries, fp.query_proofs):
        for (rows, path), bo in zip(inputs, qp.input_proof):
            assert rows == [from_mont(r) for r in bo.opened_values] and path == from_mont(bo.opening_proof)
        assert len(steps) == len(qp.commit_phase_openings)
        for (sib, path), st in zip(steps, qp.commit_phase_openings):
            assert [sib] == from_mont(st.sibling_value) and path == from_mont(st.opening_proof)


# ------------------------------------------------------------ lane forms
def _child_wires(args, env, n):
    r = subprocess.run([sys.executable, os.path.join(HERE, "pcs_gpu_child.py")] + args, capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, **env))
    wires = [x[5:] for x in r.stdout.splitlines() if x.startswith("WIRE ")]
    assert r.returncode == 0 and len(wires) == n, f"child ended with status {r.returncode}: {r.stderr[-2000:]}"
    return [bytes.fromhex(w) for w in wires]


def _child(args, env):
    return _child_wires(args, env, 1)[0]


@pytest.mark.parametrize("env", [{}, {"LSP_COOP_MAX": "16", "LSP_PAIR_MAX": "64"},
                                 {"LSP_COOP_MAX": "1", "LSP_PAIR_MAX": "1"}],
                         ids=["default", "coop16_pair64", "coop1_pair1"])
def test_roll_in_rounds_in_every_lane_form(product_lib, env):
    """the ladder from LDE height 2^10: its fused leaf batches are 256, 128, ...,
    8 leaves, so with 16/64 they run with 1, 2 and 4 lanes per leaf, with 1/1
    all with 1, by default all with 4"""
    assert _child(["case", "ladder_2e10"], env) == C.reference("ladder_2e10").wire


HOST_PATH_CASES = ["ladder", "gaps", "final_poly_len_1"]


@pytest.mark.parametrize("env", [{"LSP_HOST_TREE_TOP": "8"}, {"LSP_HOST_TREE_TOP": "4", "LSP_FRI_HOST_TAIL": "16"}],
                         ids=["top8", "top4_tail16"])
def test_roll_in_rounds_on_the_host_paths(product_lib, env):
    """The PCS runs the prover's commit phase with no host tree top and no host
    tail; the environment gives it both.  Top 8: the last trees' leaves are hashed
    on the host over a vector the plain fold kernel made with its roll-in (the
    ladder rolls in at every length down to 16).  Top 4, tail 16: the host runs the
    last rounds, and only from where no roll-in remains -- on the ladder the final
    round alone, on gaps the rounds from length 32 (its roll-in) down.  The proofs
    are the references' byte for byte."""
    wires = _child_wires(["case"] + HOST_PATH_CASES, env, len(HOST_PATH_CASES))
    for name, wire in zip(HOST_PATH_CASES, wires):
        assert wire == C.reference(name).wire, name


WIDE_LOGS = (14, 13, 12, 11, 10)  # LDE heights 2^17 ... 2^13: leaf batches of 64K ... 4K cross 32K and 16K


def wide_config():
    from linea_stark_prover_amd.prover import StarkConfig
    return StarkConfig(num_queries=C.NQ)


def wide_proof(ctx):
    """a ladder of width 2 at true widths, one point per matrix:
    (commitment, dims, z, proof bytes)"""
    from linea_stark_prover_amd.prover import HashChallenger, TwoAdicFriPcs
    rng = np.random.default_rng(1715)
    mats = []
    for lg in WIDE_LOGS:
        m = rng.integers(0, 1 << 63, size=(1 << lg, 2, 4), dtype=np.uint64)
        m[..., 3] &= np.uint64((1 << 60) - 1)  # below the modulus: any such word is an element's Montgomery form
        mats.append(m)
    pcs, ch = TwoAdicFriPcs(ctx), HashChallenger(ctx)
    root, tree = pcs.commit(mats)
    ch.observe(root)
    z = ch.sample()
    _, wire = pcs.open([(tree, [z] * len(mats))], ch)
    return root, [(1 << lg, 2) for lg in WIDE_LOGS], z, wire


def test_true_widths_equal_the_four_lane_form(product_lib):
    from linea_stark_prover_amd.prover import Context, HashChallenger, TwoAdicFriPcs
    with Context(wide_config()) as ctx:
        root, dims, z, wire = wide_proof(ctx)
        ch = HashChallenger(ctx)
        ch.observe(root)
        assert np.array_equal(ch.sample(), z)
        assert TwoAdicFriPcs(ctx).verify([(root, [(h, w, z) for h, w in dims])], wire, ch)
    # every leaf batch in the 4-lane form
    assert _child(["wide"], {"LSP_COOP_MAX": "1048576"}) == wire
