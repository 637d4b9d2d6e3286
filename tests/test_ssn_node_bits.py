"""Options node_bits / node_bits_words of the fused node pass (pantax_amd/csrc/ssn_plan.hpp: ssn_node_bits -- where node_rows_kernel takes a node's
bit-vector words from) are decided by a pure function of plain values: tests/native/ssn_node_bits_check.cpp checks it at its edges.  It is compiled here
together with ssn_plan.cpp by the host C++ compiler under AddressSanitizer and UBSan and run as a program of its own -- no GPU, no HIP, nothing loaded
into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")


def test_ssn_node_bits_native_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ssn_node_bits_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "ssn_node_bits_check.cpp"), os.path.join(CSRC, "ssn_plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "ssn_node_bits_check: ok" in run.stdout
