"""TwoAdicFriPcs over batches of unequal heights, CPU side:
the big-integer reference (tests/pcs_ref.py) tied to the committed oracle's
uni-stark proof, the product's host verifier on the reference's proofs --
accepted, and every single tamper rejected, in a child process
(tests/pcs_verify_child.py) -- the refusals on a host-only context, and the
challenger handle.  Everything is bit-exact.
"""
import ctypes
import json
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
from linea_stark_prover_amd import _lib  # noqa: E402
from linea_stark_prover_amd.field import from_mont, to_mont  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

P = O.P


# ------------------------------------------------------ uni-stark anchor
@pytest.mark.parametrize("log_h", [3, 5])
def test_reference_reproduces_the_oracles_uni_stark_open(log_h):
    """one batch [trace at zeta, zeta w_h], one batch [q width-1 chunks at zeta,
    shifts GEN g_Q^j], the challenger replayed to where pyoracle.prove calls
    open: the reference gives that proof's FRI input, betas, roots, final
    polynomial and every query's rows, paths and steps"""
    s = O.setup_from_seed()
    pp, fri = s.perm, O.FriParams()
    cfgs, cols = O.synthetic_perm_trace(log_h, 3, s.alpha, s.delta, O.DEFAULT_SEED)
    rows, pub = O.columns_to_rows(cols), [s.alpha, s.delta]
    log = {}
    want = O.prove(cfgs, rows, pub, pp, fri, trace_log=log)
    h, q = 1 << log_h, 1 << want.log_q
    gq = O.two_adic_generator(log_h + want.log_q)
    chunks = [[[log["quotient"][k * q + j]] for k in range(h)] for j in range(q)]
    trace = R.commit([rows], None, pp, fri)
    quot = R.commit(chunks, [O.GENERATOR * pow(gq, j, P) % P for j in range(q)], pp, fri)
    assert trace.ldes[0] == log["trace_lde"] and trace.tree.layers == log["trace_layers"]
    assert quot.tree.layers == log["quotient_layers"]

    ch = O.HashChallenger(pp)
    ch.observe(log_h)
    ch.observe(trace.root)
    ch.observe_slice(pub)
    assert ch.sample() == log["alpha"]
    ch.observe(quot.root)
    zeta = ch.sample()
    assert zeta == log["zeta"]
    zn = zeta * O.two_adic_generator(log_h) % P
    got = {}
    ys, proof = R.open([trace, quot], [[[zeta, zn]], [[zeta]] * q], ch, pp, fri, log=got)

    assert ys[0][0] == [want.trace_local, want.trace_next]
    assert [m[0][0] for m in ys[1]] == want.quotient_chunks
    assert got["alpha"] == log["alpha_fri"]
    assert list(got["ro"]) == [h << fri.log_blowup] and got["ro"][h << fri.log_blowup] == log["fri_input"]
    assert got["betas"] == log["betas"]
    assert proof.roots == want.fri_roots and proof.final_poly == [want.final_poly]
    assert proof.pow_witness == want.pow_witness
    assert len(proof.queries) == len(want.queries) == fri.num_queries
    for (inputs, steps), (t_row, t_path, q_row, q_path, w_steps) in zip(proof.queries, want.queries):
        assert inputs[0] == ([t_row], t_path)
        assert inputs[1] == ([[v] for v in q_row], q_path)
        assert steps == w_steps
    ch2 = O.HashChallenger(pp, initial=[])
    ch2.observe(log_h)
    ch2.observe(trace.root)
    ch2.observe_slice(pub)
    ch2.sample()
    ch2.observe(quot.root)
    ch2.sample()
    assert R.verify([trace.root, quot.root], [trace.dims(fri), quot.dims(fri)], [[[zeta, zn]], [[zeta]] * q], proof,
                    ch2, pp, fri)


def test_reference_wire_format_layout():
    ref = C.reference("smallest")
    w = ref.wire
    assert w[:8] == b"LSPPCS01"
    assert np.frombuffer(w[8:36], "<u4").tolist() == [1, C.NQ, 1, 1, 1, 1, 1]  # counts, then the one matrix
    # 1 opened value, 1 root, 1 coefficient, the witness; per query a row, 4 digests, a sibling, 3 digests
    assert len(w) == 36 + 4 * 32 + C.NQ * (32 + 4 + 4 * 32 + 32 + 4 + 3 * 32)


# ---------------------------------------------------------- host verifier
def _child(mode):
    r = subprocess.run([sys.executable, os.path.join(HERE, "pcs_verify_child.py"), mode], capture_output=True,
                       text=True, timeout=600)
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    last = lines[-1] if lines else None
    assert r.returncode == 0 and last and last["phase"] == "done", (
        f"child ended with status {r.returncode} during {last}: {r.stderr[-2000:]}")
    return {x["name"]: x for x in lines if x["phase"] == "ret"}


def test_host_verifier_accepts_the_reference_proofs(product_lib):
    rets = _child("accept")
    assert set(rets) == set(C.CASES)
    bad = {n: (x["rc"], x["check"]) for n, x in rets.items() if x["rc"] != 0}
    assert not bad, f"reference proofs rejected (status, check): {bad}"


# the check of include/lsp.h that meets each tamper first.  From a changed root,
# final polynomial or witness on, the transcript differs: the witness fails its
# 4-bit check (7) or, one time in 16, passes it and the query indices move (8).
TAMPER_CHECKS = {
    "opened value": {10}, "row element": {8}, "path digest": {8}, "sibling": {10}, "root": {7, 8},
    "final poly": {7, 8}, "pow witness": {7, 8}, "pow witness beyond 64 bits": {6}, "commitment": {8},
    "height": {2}, "height of a shorter matrix": {8}, "width": {3}, "point": {10}, "dropped roll-in height": {10},
}


def test_host_verifier_rejects_every_single_tamper(product_lib):
    rets = _child("tamper")
    assert set(rets) == set(TAMPER_CHECKS)
    for what, x in rets.items():
        assert x["rc"] == _lib.LSP_E_VERIFY and x["check"] in TAMPER_CHECKS[what], (what, x)
        assert x["ref_ok"] is False, f"the reference's verifier accepts the tamper: {what}"


def test_damaged_bytes_return_a_status(product_lib):
    rets = _child("damage")
    n = len(C.reference("two_batches_below").wire)
    assert len(rets) == n + 300
    for what, x in rets.items():
        assert x["rc"] == _lib.LSP_E_VERIFY, (what, x)  # no damaged proof verifies
        assert not x["parsed"] or x["same"], f"parsed bytes did not serialize back: {what}"
    assert not any(x["parsed"] for what, x in rets.items() if what.startswith("truncated"))
    assert any(x["parsed"] for what, x in rets.items() if what.startswith("mutation"))


# ------------------------------------------------------------- refusals
@pytest.fixture(scope="module")
def host_ctx(product_lib):
    from linea_stark_prover_amd.prover import Context, StarkConfig
    ctx = Context(StarkConfig(num_queries=C.NQ), device=-1)  # LSP_HOST_ONLY
    yield ctx
    ctx.close()


def _commit_status(ctx, dims, shifts=None):
    from linea_stark_prover_amd.prover import TwoAdicFriPcs
    buf = np.zeros((64, 4), np.uint64)  # every refusal comes before a matrix is read
    try:
        TwoAdicFriPcs(ctx).commit([buf.ctypes.data] * len(dims), shifts, dims=dims)
    except _lib.LspError as e:
        return e.code
    return 0


def test_commit_refusals_on_a_host_only_context(host_ctx):
    assert _commit_status(host_ctx, []) == _lib.LSP_E_ARG                      # no matrix
    assert _commit_status(host_ctx, [(8, 0)]) == _lib.LSP_E_ARG                # height_classes' refusals
    assert _commit_status(host_ctx, [(8, (1 << 20) + 1)]) == _lib.LSP_E_ARG
    assert _commit_status(host_ctx, [(12, 1)]) == _lib.LSP_E_SIZE
    assert _commit_status(host_ctx, [(0, 1)]) == _lib.LSP_E_SIZE
    assert _commit_status(host_ctx, [(1 << 41, 1)]) == _lib.LSP_E_SIZE
    assert _commit_status(host_ctx, [(1 << 36, 1 << 13)]) == _lib.LSP_E_SIZE   # beyond 2^48 elements
    assert _commit_status(host_ctx, [(8, 1)] * 9) == _lib.LSP_E_ARG            # a ninth matrix in a class
    assert _commit_status(host_ctx, [(8, 1), (1, 2)]) == _lib.LSP_E_SIZE       # LDE height 8 = 2^log_blowup
    assert b"LDE height below" in _lib.lib().lsp_last_error(host_ctx.h)
    assert _commit_status(host_ctx, [(8, 1)], shifts=to_mont([0])) == _lib.LSP_E_ARG
    # valid arguments: the state check
    assert _commit_status(host_ctx, [(8, 1), (2, 3)]) == _lib.LSP_E_STATE
    assert b"host-only" in _lib.lib().lsp_last_error(host_ctx.h)


def _verify_status(ctx, rounds):
    from linea_stark_prover_amd.prover import HashChallenger, TwoAdicFriPcs
    args = [(to_mont([1]), [(h, w, to_mont(zs)) for h, w, zs in b]) for b in rounds]
    try:
        TwoAdicFriPcs(ctx).verify(args, b"LSPPCS01", HashChallenger(ctx))
    except _lib.LspError as e:
        return e.code
    return _lib.LSP_E_VERIFY


def test_opening_refusals_on_a_host_only_context(host_ctx):
    z = 12345
    on_coset = O.GENERATOR * pow(O.two_adic_generator(6), 5, P) % P  # in GEN H_64, the LDE coset of 8 rows
    assert _verify_status(host_ctx, []) == _lib.LSP_E_ARG
    assert _verify_status(host_ctx, [[]]) == _lib.LSP_E_ARG                               # a batch of no matrix
    assert _verify_status(host_ctx, [[(8, 1, []), (4, 1, [])]]) == _lib.LSP_E_ARG         # no point at all
    assert _verify_status(host_ctx, [[(8, 1, []), (4, 1, [z])]]) == _lib.LSP_E_ARG        # the tallest has none
    assert _verify_status(host_ctx, [[(4, 1, [z])], [(8, 1, [])]]) == _lib.LSP_E_ARG      # ... over all batches
    assert _verify_status(host_ctx, [[(8, 1, [z]), (1, 1, [z])]]) == _lib.LSP_E_SIZE      # below 2 * 2^log_blowup
    assert _verify_status(host_ctx, [[(8, 1, [z, on_coset])]]) == _lib.LSP_E_ARG          # p3 divides by zero
    assert _verify_status(host_ctx, [[(8, 2, [z]), (4, 1, [on_coset])]]) == _lib.LSP_E_VERIFY  # not its own coset
    assert _verify_status(host_ctx, [[(12, 1, [z])]]) == _lib.LSP_E_SIZE
    assert _verify_status(host_ctx, [[(8, 0, [z])]]) == _lib.LSP_E_ARG
    assert _verify_status(host_ctx, [[(8, 1, [z])]]) == _lib.LSP_E_VERIFY                 # accepted arguments: check 1
    # lsp_pcs_open: its arguments first, and a host-only context holds no tree to get past them
    from linea_stark_prover_amd.prover import HashChallenger
    lib, ch, out = _lib.lib(), HashChallenger(host_ctx), ctypes.c_void_p()
    trees, n, pt = (ctypes.c_void_p * 1)(None), (ctypes.c_size_t * 1)(1), to_mont([z])
    assert lib.lsp_pcs_open(host_ctx.h, trees, 1, n, pt.ctypes.data, ch.handle, ctypes.byref(out)) == _lib.LSP_E_ARG
    assert lib.lsp_pcs_open(host_ctx.h, trees, 0, n, pt.ctypes.data, ch.handle, ctypes.byref(out)) == _lib.LSP_E_ARG


def test_handles_refuse_null_and_foreign_memory(product_lib):
    lib = product_lib
    assert lib.lsp_challenger_free(None) != 0 and lib.lsp_pcs_proof_free(None) != 0
    junk = ctypes.create_string_buffer(4096)  # neither a challenger nor a proof: refused by its first word
    out, n, u = np.zeros((1, 4), np.uint64), ctypes.c_size_t(), ctypes.c_uint64()
    assert lib.lsp_challenger_sample(ctypes.cast(junk, ctypes.c_void_p), out.ctypes.data) == _lib.LSP_E_ARG
    assert lib.lsp_challenger_sample_bits(ctypes.cast(junk, ctypes.c_void_p), 3, ctypes.byref(u)) == _lib.LSP_E_ARG
    assert lib.lsp_challenger_free(ctypes.cast(junk, ctypes.c_void_p)) == _lib.LSP_E_ARG
    assert lib.lsp_pcs_proof_serialize(ctypes.cast(junk, ctypes.c_void_p), None, 0, ctypes.byref(n)) == _lib.LSP_E_ARG
    assert lib.lsp_pcs_proof_free(ctypes.cast(junk, ctypes.c_void_p)) == _lib.LSP_E_ARG


# ------------------------------------------------------------ challenger
@pytest.mark.parametrize("mont", [False, True])
def test_challenger_handle_is_the_oracles_hash_challenger(product_lib, mont):
    from linea_stark_prover_amd.prover import Context, HashChallenger, StarkConfig
    ctx = Context(StarkConfig(sample_bits_montgomery=mont), device=-1)
    ch, want = HashChallenger(ctx), O.HashChallenger(C.pp(), mont_bits=mont)
    ctx.close()  # the handle holds what it needs
    vals = [3, P - 1, 0, 1 << 200]
    ch.observe(to_mont(vals[:1]))
    ch.observe(to_mont(vals[1:]))
    want.observe_slice(vals)
    assert from_mont(ch.sample()) == [want.sample()]
    assert from_mont(ch.sample()) == [want.sample()]  # an empty output buffer: flush again
    for bits in (1, 7, 33, 64):
        assert ch.sample_bits(bits) == want.sample_bits(bits)
    ch.observe(to_mont([5]))
    want.observe(5)
    assert ch.sample_bits(20) == want.sample_bits(20)


def test_opened_values_view_and_round_trip(product_lib):
    ref, lib = C.reference("classes"), product_lib
    h = ctypes.c_void_p()
    assert lib.lsp_pcs_proof_deserialize(ref.wire, len(ref.wire), ctypes.byref(h)) == 0
    vals, n = ctypes.c_void_p(), ctypes.c_size_t()
    assert lib.lsp_pcs_proof_opened_values(h, ctypes.byref(vals), ctypes.byref(n)) == 0
    flat = [v for b in ref.proof.ys for m in b for p in m for v in p]
    assert n.value == len(flat)
    got = np.ctypeslib.as_array(ctypes.cast(vals, ctypes.POINTER(ctypes.c_uint64)), (n.value, 4))
    assert from_mont(got) == flat
    ln = ctypes.c_size_t()
    assert lib.lsp_pcs_proof_serialize(h, None, 0, ctypes.byref(ln)) == 0 and ln.value == len(ref.wire)
    small = ctypes.create_string_buffer(8)
    assert lib.lsp_pcs_proof_serialize(h, small, 8, ctypes.byref(ln)) == _lib.LSP_E_ARG
    buf = ctypes.create_string_buffer(ln.value)
    assert lib.lsp_pcs_proof_serialize(h, buf, ln.value, ctypes.byref(ln)) == 0 and buf.raw == ref.wire
    assert lib.lsp_pcs_proof_free(h) == 0
