"""The host side of the staged uploads (pantax_amd/csrc/upload_host.hpp: SegFiller, StageCrew, parallel_for, the two policies that size the ring and its
crew, the ring lease) is plain C++ without a HIP include: tests/native/upload_host_check.cpp drives it over temporary files it writes itself.  It is compiled
here with upload_host.cc by the host C++ compiler, once under AddressSanitizer and UBSan and once under ThreadSanitizer (the crew's generations and the lease
are what that build is for), and run as a program of its own -- no GPU, no HIP, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")


@pytest.mark.parametrize("sanitize", [["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], ["-fsanitize=thread"]], ids=["asan_ubsan", "tsan"])
def test_upload_host_native_check(tmp_path, sanitize):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "upload_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread"] + sanitize + ["-I", CSRC, os.path.join(CSRC, "upload_host.cc"),
                    os.path.join(ROOT, "tests", "native", "upload_host_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "upload_host_check: ok" in run.stdout
