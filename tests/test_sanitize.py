"""ASan + UBSan over the host code that reads untrusted bytes (VERDICT r01
weak 10): tools/sanitize/run.sh builds liblsp_hip.so's host side with
-fsanitize=address,undefined (device code unchanged) and fuzzes the CBOR trace
parser (cbor.cpp), the proof parser and view (proof.cpp), the host verifier
(verify.cpp) and the big-endian word reader with truncations and random
mutations of a real proof and of the CBOR fixtures; and, from job files that
hold a proof with its verifier's arguments, the PCS parser and verifier
(pcs.cpp) and lsp_verify_preprocessed, which share the FRI checks (fri.cpp) and
the byte reader (wire.hpp) with them.  The driver is a program of its own;
nothing is loaded into Python.  CPU only."""
import os
import shutil
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="needs hipcc")
@pytest.mark.parametrize("log_n,ncols,seed", [(6, 3, 1), (5, 6, 2)])
def test_parsers_under_asan_ubsan(oracle_lib, tmp_path, log_n, ncols, seed):
    p = oracle_lib.setup()
    tb, w = oracle_lib.gen_perm_trace(p, log_n, ncols)
    proof = tmp_path / "proof.bin"
    proof.write_bytes(oracle_lib.prove(p, tb, 1 << log_n, w, oracle_lib.perm_air(ncols)))
    env = dict(os.environ, LSP_SAN_NCOLS=str(ncols))
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize", "run.sh"), str(proof), "400", str(seed)],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "sanitize ok" in r.stdout


def _pcs_job(name):
    """tools/sanitize/driver.cpp's "SANPCS01": a case of tests/pcs_cases.py as lsp_pcs_verify is given it"""
    import pcs_cases as C
    from linea_stark_prover_amd.field import to_mont
    ref, fri = C.reference(name), C.fri_of(name)
    commits = [c.root for c in ref.coms]
    out = bytearray(b"SANPCS01")
    out += struct.pack("<4I", fri.log_final_poly_len, fri.proof_of_work_bits, fri.num_queries, len(commits))
    for c, dims, pts in zip(commits, ref.dims(fri), ref.rounds):
        out += to_mont([c]).tobytes() + struct.pack("<I", len(dims))
        for (h, w), zs in zip(dims, pts):
            out += struct.pack("<QQI", h, w, len(zs)) + (to_mont(zs).tobytes() if zs else b"")
    out += struct.pack("<I", len(commits)) + to_mont(commits).tobytes()
    return bytes(out) + ref.wire


def _prep_job():
    """"SANPRP01": a reference LSPPRF03 proof (tests/preprocessed_ref.py) as lsp_verify_preprocessed is given it"""
    import preprocessed_ref as PR
    from linea_stark_prover_amd.field import to_mont
    from oracle import pyoracle as O
    s = O.setup_from_seed()
    fixed, main, extra = PR.build_rows("gated", 8)
    pubi = [s.alpha, s.delta] + extra
    air = PR.build_air("gated", "b")
    proof, log = PR.prove(air, main, fixed, pubi, s.perm, O.FriParams())
    desc = list(air.descriptor())
    out = bytearray(b"SANPRP01") + struct.pack("<I", len(desc)) + struct.pack("<%di" % len(desc), *desc)
    out += struct.pack("<I", len(pubi)) + to_mont(pubi).tobytes()
    out += to_mont([log["prep_root"]]).tobytes() + struct.pack("<I", 2)
    return bytes(out) + proof


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="needs hipcc")
def test_pcs_and_preprocessed_verifiers_under_asan_ubsan(oracle_lib, tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    p = oracle_lib.setup()
    tb, w = oracle_lib.gen_perm_trace(p, 5, 3)
    proof = tmp_path / "proof.bin"
    proof.write_bytes(oracle_lib.prove(p, tb, 1 << 5, w, oracle_lib.perm_air(3)))
    jobs = {"pcs.job": _pcs_job("two_batches_below"), "pcs_fp1.job": _pcs_job("final_poly_len_1"),
            "prep.job": _prep_job()}
    for name, data in jobs.items():
        (tmp_path / name).write_bytes(data)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize", "run.sh"), str(proof), "300", "3"] +
                       [str(tmp_path / name) for name in jobs], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "sanitize ok" in r.stdout


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="needs hipcc")
def test_debug_bounds_build(product_lib):
    """SURVEY 5's bounds-checked debug kernels: build.py --debug-bounds
    compiles every kernel with LSP_DEBUG_BOUNDS (csrc/dbg_bounds.hpp) into
    liblsp_hip_dbg.so, which exports the product's symbols and names itself;
    tests/test_gpu_debug_bounds.py runs it on the GPU"""
    import ctypes
    from linea_stark_prover_amd import _lib
    from linea_stark_prover_amd import build as B
    lib_path = B.build(verbose=False, debug_bounds=True)
    assert os.path.basename(lib_path) == "liblsp_hip_dbg.so"
    code = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); L.lsp_version.restype = ctypes.c_char_p; "
            "print(L.lsp_version().decode()); "
            "[getattr(L, n) for n in sys.argv[2:]]")
    r = subprocess.run([os.sys.executable, "-c", code, lib_path] + list(_lib.EXPORTED), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "debug-bounds" in r.stdout
    product_lib.lsp_version.restype = ctypes.c_char_p
    assert b"debug-bounds" not in product_lib.lsp_version()
