"""The reports named in the sized extension of the file seam (pantax_amd/csrc/report_plan.hpp: EXT_REPORTS, the third id space of the plan; the model fit
report is its first row) are planned by pure functions of plain values: tests/native/fit_report_plan_check.cpp checks them at their edges -- off values,
a missing extension, a struct_size that ends before the field or cannot be one, the refusal strings and their order, the resume truth table, and that
pantax_hip_profiling_config kept its size.  It is compiled here together with report_plan.cpp by the host C++ compiler under AddressSanitizer and UBSan
and run as a program of its own -- no GPU, no HIP, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")


def test_fit_report_plan_native_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fit_report_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "fit_report_plan_check.cpp"), os.path.join(CSRC, "report_plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "fit_report_plan_check: ok" in run.stdout
