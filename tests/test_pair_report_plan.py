"""The reports about pairs of rows of the strain table (pantax_amd/csrc/report_plan.hpp: PAIR_REPORTS, the second id space of the plan) and the four-column
mirror of the pair sums (hap_pairs_plan.hpp) are pure functions of plain values: tests/native/pair_report_plan_check.cpp checks them at their edges.  It is
compiled here together with report_plan.cpp and hap_pairs_plan.cpp by the host C++ compiler under AddressSanitizer and UBSan and run as a program of its
own -- no GPU, no HIP, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")


def test_pair_report_plan_native_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pair_report_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "pair_report_plan_check.cpp"), os.path.join(CSRC, "report_plan.cpp"),
                    os.path.join(CSRC, "hap_pairs_plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "pair_report_plan_check: ok" in run.stdout
