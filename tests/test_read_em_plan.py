"""The host side of pantax_hip_strain_read_em -- how many slots the class table of a species gets and how a table that overflowed grows, which classes
the report prints (pantax_amd/csrc/read_em_plan.hpp) and the helper of the estimate -- is pure functions of plain values: tests/native/read_em_check.cpp
checks them at their edges (K = 1, 6, 7, 63, 64; read_class_slots 1 and 2^31; the bound of the growth; ties and J below, at and above N in the ranking; the
helper on the cases done by hand) and the report's row in the plan of the file seam (pantax_hip_profile_ext5 behind the 64-byte fourth version: offsets 64,
72, 80, size 88, the table's one row).  It is compiled here together with read_em_plan.cpp and report_plan.cpp by the host C++ compiler under
AddressSanitizer and UBSan, with contraction off, and run as a program of its own -- no GPU, no HIP, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")


def test_read_em_plan_native_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "read_em_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "native", "read_em_check.cpp"), os.path.join(CSRC, "read_em_plan.cpp"),
                    os.path.join(CSRC, "report_plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "read_em_check: ok" in run.stdout
