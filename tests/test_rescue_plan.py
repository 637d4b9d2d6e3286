"""The host side of pantax_hip_strain_read_rescue -- the classes of one walk (pantax_hip_rescue_walk, the C statement of the contract), the order in which
a species' candidates are printed (pantax_hip_rescue_rank), the candidate list of the file seam (pantax_amd/csrc/rescue_plan.hpp) -- is pure functions
of plain values: tests/native/rescue_check.cpp holds them on cases done by hand (the six outcomes, K = 0, J = 0, words with bit 63 set, ignored high
bits, the refusals, the rank order and its ties, the candidate cut: ranked first, then ascending, 64 - K), and the report's row in the plan of the file
seam (pantax_hip_profile_ext8 behind the 136-byte seventh version: offsets 136 and 144, size 152, the table's one row).  It is compiled here together
with rescue_plan.cpp and report_plan.cpp by the host C++ compiler under AddressSanitizer and UBSan and run as a program of its own -- no GPU, no HIP,
nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")


def test_rescue_plan_native_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rescue_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "native", "rescue_check.cpp"), os.path.join(CSRC, "rescue_plan.cpp"),
                    os.path.join(CSRC, "report_plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "rescue_check: ok" in run.stdout
