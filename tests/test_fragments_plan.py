"""The host side of the fragment support -- the fragment key of a read id (pantax_hip_fragment_key; pantax_amd/csrc/fragments_plan.hpp) -- is a pure
function of plain values: tests/native/fragments_plan_check.cpp holds it on ids done by hand (a/1, a/2, /1, x/3, ab, a/, the empty id, bytes above 127,
the refusals), and the report's row in the plan of the file seam (pantax_hip_profile_ext11 behind the 200-byte tenth version: offset 200, size 208,
the table's one row).  It is compiled here together with fragments_plan.cpp and report_plan.cpp by the host C++ compiler under AddressSanitizer and
UBSan and run as a program of its own -- no GPU, no HIP, nothing loaded into Python.  The ids handed to it on the command line come back with their key
and tag, which must be those of the Python restatement (tests/fragments_ref.py) and, for tag 0, the id hash of the tokenizers
(tests.helpers.gaf_id_hash)."""
import os
import shutil
import subprocess

import numpy as np

from tests import fragments_ref as ref
from tests.helpers import gaf_id_hash

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")


def test_fragments_plan_native_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fragments_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "native", "fragments_plan_check.cpp"), os.path.join(CSRC, "fragments_plan.cpp"),
                    os.path.join(CSRC, "report_plan.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(11)
    ids = [b"a/1", b"a/2", b"/1", b"x/3", b"ab", b"a/", b"", b"abc", b"S0R4970856/2", b"S0R4970856/1", b"S0R4970856", b"a/1/2", b"\xff/1", b"1/1", b"//1"]
    for _ in range(40):                                                       # random bytes, every third with a suffix
        n = int(rng.integers(0, 24))
        b = bytes(rng.integers(0, 256, size=n, dtype=np.uint8).tolist())
        ids.append(b + [b"", b"/1", b"/2"][len(ids) % 3])
    run = subprocess.run([exe] + [i.hex() if i else "-" for i in ids], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "fragments_plan_check: ok" in run.stdout
    got = [l.split()[1:] for l in run.stdout.splitlines() if l.startswith("key ")]
    assert len(got) == len(ids)
    tags = set()
    for i, (k, t) in zip(ids, got):
        key, tag = ref.fragment_key(i)
        assert (int(k, 16), int(t)) == (key, tag), i
        if tag == 0:
            assert int(k, 16) == gaf_id_hash(i), i
        else:
            assert int(k, 16) == gaf_id_hash(i[:-2]), i
        tags.add(tag)
    assert tags == {0, 1, 2}
