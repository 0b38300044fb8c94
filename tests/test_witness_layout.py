"""The witness blocks' column layout (csrc/witness_layout.hpp): the named
columns are 0 .. width - 1 in the documented order, the raw offsets tile the
raw block, describe() writes desc_len() words that air_walk.hpp's air_decode
reads back as the same ids shifted by col0, and the quoted widths (14, 18, 184)
hold.  Neither header has HIP types in it, so the check
(tests/witness_layout_check.cpp) is built with the host compiler alone and run
-- plainly, and under the address and undefined-behaviour sanitizers: no GPU,
no library load."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_layout_properties(tmp_path, flags):
    cxx = (os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
           or shutil.which("clang++", path="/opt/rocm/lib/llvm/bin"))
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "witness_layout_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I",
                    os.path.join(ROOT, "linea_stark_prover_amd", "csrc"),
                    os.path.join(ROOT, "tests", "witness_layout_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("104 blocks, 0 failure(s)")
