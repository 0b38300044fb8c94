"""The coset LDE's pass plan (csrc/ntt_plan.hpp) holds its invariants at every
size: stage coverage of the inverse and forward halves, tile and LDS limits,
launch geometry, and the flagship shape's plan.  The header has no HIP types in
it, so the check (tests/ntt_plan_check.cpp) is built with the host compiler
alone and run: no GPU, no library load."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_invariants(tmp_path):
    cxx = (os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
           or shutil.which("clang++", path="/opt/rocm/lib/llvm/bin"))
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ntt_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "linea_stark_prover_amd", "csrc"),
                    os.path.join(ROOT, "tests", "ntt_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("0 failure(s)")
