"""The host side of pantax_hip_strain_segments -- how the per-tile summaries of the first pass are stitched into runs that cross tile borders, which output
slot every kept run gets (pantax_amd/csrc/segments_plan.hpp) and the chain helper -- is pure functions of plain values: tests/native/segments_check.cpp
plays the device with a CPU summariser of one tile, stitches class strings by hand and at random at tile sizes of 1, 2, 16 and 1 024 against a direct
run-length pass (a walk of one tile, every tile a whole run, a lead and a trail of different classes, a run that ends exactly at a tile's last step, a walk
that begins mid-tile), and holds the report's row in the plan of the file seam (pantax_hip_profile_ext6 behind the 88-byte fifth version: offsets 88, 96,
104, 112, size 120, the table's one row).  It is compiled here together with segments_plan.cpp and report_plan.cpp by the host C++ compiler under
AddressSanitizer and UBSan and run as a program of its own -- no GPU, no HIP, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")


def test_segments_plan_native_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "segments_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "native", "segments_check.cpp"), os.path.join(CSRC, "segments_plan.cpp"),
                    os.path.join(CSRC, "report_plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "segments_check: ok" in run.stdout
