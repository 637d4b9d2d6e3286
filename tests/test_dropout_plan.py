"""The host side of pantax_hip_strain_dropout -- how many rounds of leave-one-out LPs share the device at once, where an entry and its x block sit in the
outputs, how the rows are cut into slices (pantax_amd/csrc/dropout_plan.hpp) and the substitute helper -- is pure functions of plain values:
tests/native/dropout_plan_check.cpp checks them at their edges (one round, a cap below, at and above one round, no pattern, u64 sizes, K in {0, 1, 64, 65},
ties, no positive gain, K = 1) and the report's row in the plan of the file seam (pantax_hip_profile_ext3 behind the 40-byte second version).  It is
compiled here together with dropout_plan.cpp and report_plan.cpp by the host C++ compiler under AddressSanitizer and UBSan and run as a program of its own
-- no GPU, no HIP, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")


def test_dropout_plan_native_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "dropout_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "dropout_plan_check.cpp"), os.path.join(CSRC, "dropout_plan.cpp"), os.path.join(CSRC, "report_plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "dropout_plan_check: ok" in run.stdout
