"""Child process of tests/test_preprocessed_verify.py: truncations and seeded
single-byte mutations of a reference LSPPRF03 proof through
lsp_proof_deserialize and lsp_verify_preprocessed on a host-only context.  One JSON line goes out before
each call, so a crash names its input; the last line holds the verdict counts."""
import ctypes
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import preprocessed_ref as PR  # noqa: E402
from linea_stark_prover_amd import _lib as L  # noqa: E402
from linea_stark_prover_amd.field import to_mont  # noqa: E402
from linea_stark_prover_amd.prover import Context, StarkConfig  # noqa: E402
from oracle import pyoracle as O  # noqa: E402


def main():
    s = O.setup_from_seed()
    fixed, main_rows, extra = PR.build_rows("gated", 2)
    pubi = [s.alpha, s.delta] + extra
    air = PR.build_air("gated", "b")
    proof, log = PR.prove(air, main_rows, fixed, pubi, s.perm)
    ctx = Context(StarkConfig(), device=-1)
    pub, pre = to_mont(pubi), (to_mont([log["prep_root"]]), 2)
    assert ctx.verify(proof, air, pub, preprocessed=pre)
    counts = {"accepted": 0, "rejected": 0, "parsed": 0, "unparsed": 0}

    def load(data):
        """lsp_proof_deserialize: a status, and what parses serializes back to the same bytes"""
        h = ctypes.c_void_p()
        rc = L.lib().lsp_proof_deserialize(data, len(data), ctypes.byref(h))
        assert rc in (L.LSP_OK, L.LSP_E_ARG), rc
        if rc != L.LSP_OK:
            return False
        try:
            n = ctypes.c_size_t()
            assert L.lib().lsp_proof_serialize(h, None, 0, ctypes.byref(n)) == L.LSP_OK and n.value == len(data)
            buf = ctypes.create_string_buffer(n.value)
            assert L.lib().lsp_proof_serialize(h, buf, n.value, ctypes.byref(n)) == L.LSP_OK
            assert buf.raw[:n.value] == data
        finally:
            L.lib().lsp_proof_free(h)
        return True

    def run(kind, where, data):
        print(json.dumps({"case": kind, "at": where}), flush=True)
        counts["parsed" if load(data) else "unparsed"] += 1
        try:
            ok = ctx.verify(data, air, pub, preprocessed=pre)
        except L.LspError as e:  # a status all the same
            assert e.code in (L.LSP_E_ARG, L.LSP_E_VERIFY), e
            ok = False
        counts["accepted" if ok else "rejected"] += 1
        return ok

    assert load(proof)
    for n in list(range(0, 420)) + list(range(420, len(proof), 61)):
        assert not run("truncate", n, proof[:n]) and counts["parsed"] == 0
    assert not run("extend", len(proof), proof + b"\0")
    rng = random.Random(2025)
    for _ in range(300):
        k, bit = rng.randrange(len(proof)), 1 << rng.randrange(8)
        data = bytearray(proof)
        data[k] ^= bit
        assert not run("flip", [k, bit], bytes(data))
    print(json.dumps({"done": True, **counts}), flush=True)


if __name__ == "__main__":
    main()
