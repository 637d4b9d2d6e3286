"""The host side of pantax_hip_strain_bootstrap -- how many replicates share the device at once (pantax_amd/csrc/bootstrap_plan.hpp), the summary over
replicates and the weight helper -- is pure functions of plain values: tests/native/bootstrap_plan_check.cpp checks them at their edges (one replicate, a
cap below, at and above one replicate, no rows, u64 sizes, the table's borders, 10^6 weights against Poisson(1)) and the report's row in the plan of
the file seam (pantax_hip_profile_ext2 behind the 16-byte first version).  It is compiled here together with bootstrap_plan.cpp and report_plan.cpp by the host C++ compiler under AddressSanitizer and UBSan and run as a program of its own -- no GPU, no HIP, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")


def test_bootstrap_plan_native_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "bootstrap_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "bootstrap_plan_check.cpp"), os.path.join(CSRC, "bootstrap_plan.cpp"), os.path.join(CSRC, "report_plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "bootstrap_plan_check: ok" in run.stdout
