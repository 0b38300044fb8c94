"""Child process of tests/test_gpu_pcs.py's lane-form tests: the lane knobs
(LSP_COOP_MAX, LSP_PAIR_MAX) are read once per process, so each setting proves
in a process of its own and prints the proof's bytes in hex.

    python tests/pcs_gpu_child.py case NAME... # cases of tests/pcs_cases.py, one WIRE line each
    python tests/pcs_gpu_child.py wide         # the ladder at true widths (test_gpu_pcs.wide_proof)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import pcs_cases as C  # noqa: E402
import test_gpu_pcs as T  # noqa: E402
from linea_stark_prover_amd.prover import Context  # noqa: E402


def main():
    if sys.argv[1] == "wide":
        with Context(T.wide_config()) as ctx:
            print("WIRE " + T.wide_proof(ctx)[3].hex(), flush=True)
        return
    for name in sys.argv[2:]:
        with Context(C.stark_config(name)) as ctx:
            print("WIRE " + T.gpu_open(ctx, name)[2].hex(), flush=True)


if __name__ == "__main__":
    main()
