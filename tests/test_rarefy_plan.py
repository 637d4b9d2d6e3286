"""The host side of pantax_hip_strain_rarefy -- the cut of a replicate's levels into passes over the reads (rarefy_plan, pantax_amd/csrc/rarefy_plan.hpp),
the entry of a (replicate, level) and the depth rule's host helper -- is pure functions of plain values: tests/native/rarefy_check.cpp holds them at their
edges, and the report's row in the plan of the file seam (pantax_hip_profile_ext10 behind the 168-byte ninth version: offsets 168 .. 192, size 200, the
table's one row, the defaults 5 / 5 / 42 and the refusals).  It is compiled here together with rarefy_plan.cpp and report_plan.cpp by the host C++
compiler under AddressSanitizer and UBSan and run as a program of its own -- no GPU, no HIP, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")


def test_rarefy_plan_native_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rarefy_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "native", "rarefy_check.cpp"), os.path.join(CSRC, "rarefy_plan.cpp"),
                    os.path.join(CSRC, "report_plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "rarefy_check: ok" in run.stdout
