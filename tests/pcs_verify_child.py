"""Child process of tests/test_pcs.py: the product's host verifier
(lsp_pcs_verify on a host-only context) and lsp_pcs_proof_deserialize on
reference proofs, tampered proofs and damaged bytes.  One JSON line per call,
the "call" line before it, so a crash names the call that faulted.

    python tests/pcs_verify_child.py accept    # every case's reference proof
    python tests/pcs_verify_child.py tamper    # single tampers of one proof
    python tests/pcs_verify_child.py damage    # truncations, byte mutations
"""
import copy
import ctypes
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import pcs_cases as C  # noqa: E402
import pcs_ref as R  # noqa: E402
from linea_stark_prover_amd import _lib  # noqa: E402
from linea_stark_prover_amd.field import to_mont  # noqa: E402
from linea_stark_prover_amd.prover import Context, HashChallenger, TwoAdicFriPcs  # noqa: E402

TAMPER_CASE = "two_batches_below"


def say(**kw):
    print(json.dumps(kw), flush=True)


def product_verify(ctx, name, commits, dims, rounds, wire, observed=None):
    """(status, failing check) of lsp_pcs_verify after the case's transcript
    (observed: the commitments that went into it, when not `commits`)"""
    ch = HashChallenger(ctx)
    ch.observe(to_mont(observed or commits))
    ch.sample()
    pcs = TwoAdicFriPcs(ctx)
    args = [(to_mont([c]), [(h, w, to_mont(zs)) for (h, w), zs in zip(d, pts)])
            for c, d, pts in zip(commits, dims, rounds)]
    try:
        ok = pcs.verify(args, wire, ch)
        return (0 if ok else _lib.LSP_E_VERIFY), pcs.last_check
    except _lib.LspError as e:
        return e.code, 0


def tampers(ref, fri):
    """name -> (commits, dims, rounds, proof), each one change away from the reference's"""
    base = ([c.root for c in ref.coms], ref.dims(fri), ref.rounds, ref.proof)

    def make(f):
        commits, dims, rounds, proof = copy.deepcopy(base)
        box = {"commits": commits, "dims": dims, "rounds": rounds, "proof": proof}
        f(box)
        return box["commits"], box["dims"], box["rounds"], box["proof"]

    def bump(lst, i):
        lst[i] = (lst[i] + 1) % C.P

    def drop_roll_in(b):  # batch 1's matrix of height 16 loses its points, in the proof and for the verifier alike
        b["rounds"][1][1] = []
        b["proof"].ys[1][1] = []
        b["proof"].shape[1][1] = (b["proof"].shape[1][1][0], 0)

    def set_dim(b, batch, mat, h=None, w=None):
        hh, ww = b["dims"][batch][mat]
        b["dims"][batch][mat] = (h or hh, w or ww)

    return {
        "opened value": make(lambda b: bump(b["proof"].ys[0][0][0], 0)),
        "row element": make(lambda b: bump(b["proof"].queries[0][0][0][0][0], 0)),
        "path digest": make(lambda b: bump(b["proof"].queries[1][0][1][1], 0)),
        "sibling": make(lambda b: b["proof"].queries[0][1].__setitem__(
            0, ((b["proof"].queries[0][1][0][0] + 1) % C.P, b["proof"].queries[0][1][0][1]))),
        "root": make(lambda b: bump(b["proof"].roots, 1)),
        "final poly": make(lambda b: bump(b["proof"].final_poly, 0)),
        "pow witness": make(lambda b: setattr(b["proof"], "pow_witness", b["proof"].pow_witness + 1)),
        "pow witness beyond 64 bits": make(lambda b: setattr(b["proof"], "pow_witness", 1 << 64)),
        "commitment": make(lambda b: bump(b["commits"], 1)),
        "height": make(lambda b: set_dim(b, 0, 0, h=64)),
        "height of a shorter matrix": make(lambda b: set_dim(b, 0, 1, h=16)),
        "width": make(lambda b: set_dim(b, 0, 0, w=3)),
        "point": make(lambda b: bump(b["rounds"][1][0], 0)),
        "dropped roll-in height": make(drop_roll_in),
    }


def main():
    mode = sys.argv[1]
    lib = _lib.lib()
    ctxs = {}

    def ctx_of(name):
        if name not in ctxs:
            ctxs[name] = Context(C.stark_config(name), device=-1)  # LSP_HOST_ONLY
        return ctxs[name]

    if mode == "accept":
        for name in C.CASES:
            ref, fri = C.reference(name), C.fri_of(name)
            say(phase="call", name=name)
            rc, check = product_verify(ctx_of(name), name, [c.root for c in ref.coms], ref.dims(fri), ref.rounds,
                                       ref.wire)
            say(phase="ret", name=name, rc=rc, check=check)
    elif mode == "tamper":
        ref, fri = C.reference(TAMPER_CASE), C.fri_of(TAMPER_CASE)
        true_roots = [c.root for c in ref.coms]  # the transcript holds the prover's commitments throughout
        for what, (commits, dims, rounds, proof) in tampers(ref, fri).items():
            say(phase="call", name=what)
            rc, check = product_verify(ctx_of(TAMPER_CASE), TAMPER_CASE, commits, dims, rounds, R.serialize(proof),
                                       observed=true_roots)
            # the reference's own verifier on the same tamper
            ch, _ = C.challenger(TAMPER_CASE, true_roots)
            try:
                ref_ok = R.verify(commits, dims, rounds, proof, ch, C.pp(), fri)
            except AssertionError:  # (dimensions its tree refuses)
                ref_ok = False
            say(phase="ret", name=what, rc=rc, check=check, ref_ok=ref_ok)
    else:
        ref, fri = C.reference(TAMPER_CASE), C.fri_of(TAMPER_CASE)
        commits, dims = [c.root for c in ref.coms], ref.dims(fri)
        rnd = random.Random(20260)
        damaged = [("truncated to %d" % n, ref.wire[:n]) for n in range(len(ref.wire))]
        for k in range(300):
            b = bytearray(ref.wire)
            pos = rnd.randrange(len(b))
            b[pos] ^= 1 << rnd.randrange(8)
            damaged.append(("mutation %d at %d" % (k, pos), bytes(b)))
        for what, wire in damaged:
            say(phase="call", name=what)
            rc, check = product_verify(ctx_of(TAMPER_CASE), TAMPER_CASE, commits, dims, ref.rounds, wire)
            # what parses serializes back to the same bytes
            h, same = ctypes.c_void_p(), None
            drc = lib.lsp_pcs_proof_deserialize(wire, len(wire), ctypes.byref(h))
            if drc == 0:
                n = ctypes.c_size_t()
                assert lib.lsp_pcs_proof_serialize(h, None, 0, ctypes.byref(n)) == 0
                buf = ctypes.create_string_buffer(n.value)
                assert lib.lsp_pcs_proof_serialize(h, buf, n.value, ctypes.byref(n)) == 0
                same = buf.raw[:n.value] == wire
                assert lib.lsp_pcs_proof_free(h) == 0
            say(phase="ret", name=what, rc=rc, check=check, parsed=drc == 0, same=same)
    say(phase="done")


if __name__ == "__main__":
    main()
