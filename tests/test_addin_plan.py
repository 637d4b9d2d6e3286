"""The host side of pantax_hip_strain_addin -- how many rounds of add-one LPs share the device at once, where an entry and its x block sit in the outputs,
which instance of the objective pass takes a species and how its rows are cut into slices (pantax_amd/csrc/addin_plan.hpp) and the donor helper -- is pure
functions of plain values: tests/native/addin_plan_check.cpp checks them at their edges (J = 0, K = 0, W = 64 and 65, a cap below, at and above one round,
no pattern, u64 sizes, donor ties, no positive loss, K = 0) and the report's row in the plan of the file seam (pantax_hip_profile_ext4 behind the 48-byte
third version: offset 48, size 64, the table's one row).  It is compiled here together with addin_plan.cpp and report_plan.cpp by the host C++ compiler
under AddressSanitizer and UBSan and run as a program of its own -- no GPU, no HIP, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")


def test_addin_plan_native_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "addin_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "addin_plan_check.cpp"), os.path.join(CSRC, "addin_plan.cpp"), os.path.join(CSRC, "report_plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "addin_plan_check: ok" in run.stdout
