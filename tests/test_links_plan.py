"""The host side of pantax_hip_strain_links -- the classes of one walk's crossings (pantax_hip_link_crossings, the C statement of the contract) and the
order in which a strain's breaks are printed (pantax_hip_link_top; pantax_amd/csrc/links_plan.hpp) -- is pure functions of plain values:
tests/native/links_check.cpp holds them on cases done by hand (the four classes, K = 0, K = 64 with bit 63, ignored high bits, the refusals, the top
order and its ties), and the report's row in the plan of the file seam (pantax_hip_profile_ext9 behind the 152-byte eighth version: offsets 152 and
160, size 168, the table's one row).  It is compiled here together with links_plan.cpp and report_plan.cpp by the host C++ compiler under
AddressSanitizer and UBSan and run as a program of its own -- no GPU, no HIP, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")


def test_links_plan_native_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "links_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "native", "links_check.cpp"), os.path.join(CSRC, "links_plan.cpp"),
                    os.path.join(CSRC, "report_plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "links_check: ok" in run.stdout
