"""The host slice's plan (csrc/host_slice.hpp): no slice below 2^21 leaves unless
forced, the slice is the last aligned subtree, prefix and slice add up to every
layer for log n = 6..26 and every forced log_frac, and the 0.85 rule falls back
to a smaller fraction, then to none.  The header has no HIP types in it, so the
check (tests/host_slice_check.cpp) is built with the host compiler alone and
run -- plainly, and under the address and undefined-behaviour sanitizers: no
GPU, no library load."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_plan_properties(tmp_path, flags):
    cxx = (os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
           or shutil.which("clang++", path="/opt/rocm/lib/llvm/bin"))
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "host_slice_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I",
                    os.path.join(ROOT, "linea_stark_prover_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_slice_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("0 failure(s)")
