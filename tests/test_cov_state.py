"""The lifecycle of the coverage arena and of the unique-trio index (pantax_amd/csrc/cov_state.hpp: CovState, TrioState, cov_clean_plan) is host-only code
over plain values: tests/native/cov_state_check.cpp drives the two types and a transcription of the flags they replaced through every sequence of up to
five events, and checks cov_clean_plan at its edges.  It is compiled here by the host C++ compiler under AddressSanitizer and UBSan and run as a program of
its own -- no GPU, no HIP, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")


def test_cov_state_native_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "cov_state_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "cov_state_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "cov_state_check: ok" in run.stdout
