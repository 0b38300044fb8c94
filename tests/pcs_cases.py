"""The PCS shapes tests/test_pcs.py (host verifier, CPU) and
tests/test_gpu_pcs.py (prover, GPU) share, and their reference proofs from
tests/pcs_ref.py, each computed once per process.  No tests in this module.

A case is a list of batches, a batch a list of (height, width, shift, points)
with points 0, 1 (z) or 2 (z and z * w_height).  The transcript of a case:
observe every batch's commitment in order, sample z, open.
"""
import functools
import os
import random
import sys
from dataclasses import dataclass

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import pcs_ref as R  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

P = O.P
NQ = 5  # queries per proof: each is checked the same way, and the reference is big integers
G16 = O.two_adic_generator(4)


def _ladder(top, widths=(1, 2, 3, 7)):
    """heights top, top / 2, ..., 2: every round rolls in; one or two points per matrix"""
    hs = []
    h = top
    while h >= 2:
        hs.append(h)
        h //= 2
    return [[(h, widths[k % len(widths)], 1, 1 + k % 2) for k, h in enumerate(hs)]]


# name -> (batches, FriParams overrides)
CASES = {
    "smallest": ([[(2, 1, 1, 1)]], {}),
    "ladder": (_ladder(64), {}),
    "gaps": ([[(64, 2, 1, 2), (4, 3, 1, 1)]], {}),
    # classes of three, two and two matrices, in unsorted caller order
    "classes": ([[(8, 2, 1, 1), (32, 1, 1, 2), (16, 2, 1, 1), (8, 3, 1, 2), (32, 2, 1, 1), (16, 1, 1, 1),
                  (8, 1, 1, 1)]], {}),
    # shared heights, so the per-height power of alpha runs across the batches
    # (with a proof of work, for the tampers of tests/test_pcs.py)
    "two_batches_below": ([[(32, 2, 1, 2), (8, 1, 1, 1)], [(8, 3, 1, 1), (16, 1, 1, 2)]], {"proof_of_work_bits": 4}),
    "two_batches_above": ([[(8, 2, 1, 1), (16, 1, 1, 2)], [(32, 1, 1, 2), (8, 2, 1, 1), (16, 3, 1, 1)]], {}),
    "matrix_without_points": ([[(32, 2, 1, 1), (32, 1, 1, 0), (8, 1, 1, 2)]], {}),
    "class_without_points": ([[(32, 2, 1, 2), (16, 3, 1, 0), (8, 1, 1, 1)]], {}),
    "shifts": ([[(16, 2, 5, 2), (4, 1, O.GENERATOR * G16 % P, 1), (16, 1, O.GENERATOR, 1)]], {}),
    "final_poly_len_1": ([[(16, 2, 1, 2), (8, 1, 1, 1), (4, 3, 1, 1)]], {"log_final_poly_len": 1}),
    "pow_5_bits": ([[(8, 2, 1, 1), (4, 1, 1, 2)]], {"proof_of_work_bits": 5}),
    "u7_opened_values": ([[(8, 2, 1, 2), (4, 1, 1, 1)]], {"observe_opened_values": True}),
    "u8_montgomery_bits": ([[(8, 2, 1, 1), (4, 3, 1, 1)]], {"sample_bits_montgomery": True, "proof_of_work_bits": 3}),
    # the lane forms' ladder: LDE heights 2^10 ... 2^4
    "ladder_2e10": (_ladder(128, widths=(1, 2)), {}),
}


def fri_of(name):
    return O.FriParams(num_queries=NQ, **CASES[name][1])


def stark_config(name, **more):
    from linea_stark_prover_amd.prover import StarkConfig
    return StarkConfig(num_queries=NQ, **CASES[name][1], **more)  # (the overridden fields have FriParams' names)


@functools.lru_cache(maxsize=None)
def pp():
    return O.setup_from_seed().perm


@functools.lru_cache(maxsize=None)
def matrices(name):
    """[batch][matrix] -> rows of canonical values, seeded by the case's name"""
    rnd = random.Random("pcs " + name)
    return [[[[rnd.randrange(P) for _ in range(w)] for _ in range(h)] for h, w, _, _ in b] for b in CASES[name][0]]


def points_of(name, z):
    return [[[z, z * O.two_adic_generator(O.log2_strict(h)) % P][:n] for h, _, _, n in b] for b in CASES[name][0]]


@dataclass
class Reference:
    coms: list       # pcs_ref.Committed per batch
    z: int
    rounds: list     # [batch][matrix] -> points
    proof: R.Proof
    wire: bytes
    state: tuple     # the challenger's buffers when open returned

    def dims(self, fri):
        return [c.dims(fri) for c in self.coms]


def challenger(name, roots):
    """the case's transcript up to the points: (challenger, z)"""
    ch = O.HashChallenger(pp(), mont_bits=fri_of(name).sample_bits_montgomery)
    ch.observe_slice(roots)
    return ch, ch.sample()


@functools.lru_cache(maxsize=None)
def reference(name) -> Reference:
    fri = fri_of(name)
    coms = [R.commit(ms, [s for _, _, s, _ in b], pp(), fri) for ms, b in zip(matrices(name), CASES[name][0])]
    ch, z = challenger(name, [c.root for c in coms])
    rounds = points_of(name, z)
    _, proof = R.open(coms, rounds, ch, pp(), fri)
    return Reference(coms, z, rounds, proof, R.serialize(proof), (tuple(ch.input_buffer), tuple(ch.output_buffer)))
