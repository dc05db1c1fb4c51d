"""Host-only checks of the knob table's readers, of the HIP-free parts of the host-batch ring and of
the scratch slicing rules (csrc/rs_env.hpp, csrc/rs_host_ring.hpp, csrc/rs_slices.hpp):
tests/host/ring_main.cpp, built as a plain C++ program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reed-solomon-cc_amd", "csrc")


def _clangxx():
    for cand in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if os.path.exists(cand):
            return cand
    return shutil.which("amdclang++")


def test_ring_main(tmp_path):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("ROCm's clang++ not found")
    exe = str(tmp_path / "ring_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-pthread", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "ring_main.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RS_AMD_")}
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ring_main: ok" in r.stdout
