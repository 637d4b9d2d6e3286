"""The per-strain reports of the file seam as one table (pantax_amd/csrc/report_plan.hpp: REPORTS, plan_reports, resume_reports) are pure functions of
plain values: tests/native/report_plan_check.cpp checks them at their edges, the refusal texts against literal strings.  It is compiled here together with
report_plan.cpp by the host C++ compiler under AddressSanitizer and UBSan and run as a program of its own -- no GPU, no HIP, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")


def test_report_plan_native_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "report_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "report_plan_check.cpp"), os.path.join(CSRC, "report_plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "report_plan_check: ok" in run.stdout
