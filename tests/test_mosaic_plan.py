"""The host side of pantax_hip_strain_mosaic -- the greedy cut of one walk (pantax_hip_mosaic_walk, the C statement of the contract), the junctions a
report prints (pantax_hip_mosaic_top), the sort and run-length of the device's break records (pantax_amd/csrc/mosaic_plan.hpp) -- is pure functions of
plain values: tests/native/mosaic_check.cpp holds them on cases done by hand (one break, a break at the first possible step, the late break, foreign
steps, words with bit 63 set, a walk of 64 breaks, a cap that is too small, an empty walk, the refusals), the cut against a brute-force minimum and the
reversed walk at random, and the report's row in the plan of the file seam (pantax_hip_profile_ext7 behind the 120-byte sixth version: offsets 120 and
128, size 136, the table's one row).  It is compiled here together with mosaic_plan.cpp and report_plan.cpp by the host C++ compiler under
AddressSanitizer and UBSan and run as a program of its own -- no GPU, no HIP, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")


def test_mosaic_plan_native_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "mosaic_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "native", "mosaic_check.cpp"), os.path.join(CSRC, "mosaic_plan.cpp"),
                    os.path.join(CSRC, "report_plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "mosaic_check: ok" in run.stdout
