"""The host side of the replication index report -- the fit over the own-node windows of one strain (pantax_hip_growth_fit; pantax_amd/csrc/growth_plan.hpp)
-- is a pure function of plain values: tests/native/growth_plan_check.cpp holds it on windows done by hand, reaches every status and every refusal, and
holds the report's row in the plan of the file seam (pantax_hip_profile_ext12 behind the 208-byte eleventh version: offsets 208 .. 232, size 240).  It is
compiled here together with growth_plan.cpp and report_plan.cpp by the host C++ compiler under AddressSanitizer and UBSan and run as a program of its own
-- no GPU, no HIP, nothing loaded into Python.  The cases handed to it in a file come back with their results, which must be those of the Python
restatement (tests/growth_ref.py): integers and the status exactly, floats at relative 1e-12 -- both sides take the same operations in the same order
and only libm's log2 / exp2 may differ in the last place."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import growth_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantax_amd", "csrc")
INTS = ("n_kept", "n_zero", "n_f", "n_fit", "own_len")
FLOATS = ("median_depth", "slope", "intercept", "r2", "index")
REL = 1e-12


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("growth_plan") / "growth_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "native", "growth_plan_check.cpp"), os.path.join(CSRC, "growth_plan.cpp"),
                    os.path.join(CSRC, "report_plan.cpp"), "-o", out], check=True)
    return out


def _run(exe, tmp_path, cases):
    """cases: (len_own, bases_own, min_own, trim, min_windows, min_depth) -> per case the program's output line, split (None where it refused)"""
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for ln, bs, min_own, trim, min_windows, min_depth in cases:
            f.write(" ".join(str(x) for x in [min_own, trim, min_windows, repr(float(min_depth)), len(ln)] + [int(v) for v in ln] + [int(v) for v in bs]) + "\n")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    print(run.stdout[-2000:], run.stderr)
    assert run.returncode == 0, run.stderr
    assert "growth_plan_check: ok" in run.stdout
    lines = [l.split() for l in run.stdout.splitlines() if l.startswith("fit ")]
    assert len(lines) == len(cases)
    return [None if l[1] == "refused" else l[1:] for l in lines]


def _same(got, exp):
    assert [int(x) for x in got[:5]] == [exp[k] for k in INTS] and got[10] == exp["status"], (got, exp)
    for x, k in zip(got[5:10], FLOATS):
        g = float.fromhex(x)
        assert g == exp[k] or abs(g - exp[k]) <= REL * abs(exp[k]), (k, g, exp[k])


def _random_case(rng, kind):
    n = int(rng.integers(0, 400))
    ln = rng.integers(1, 6000, size=n)
    if kind == 0:                                                            # a sample of uneven depth, windows without bases, outliers
        bs = (ln * rng.gamma(4.0, 8.0, size=n)).astype(np.int64) * (rng.random(n) > 0.1)
        bs[rng.random(n) < 0.03] *= 500
    elif kind == 1:                                                          # shallow: many ties and zeros
        bs = rng.integers(0, 4, size=n) * ln
    else:                                                                    # one depth throughout
        bs = 7 * ln
    return (ln, bs, int(rng.integers(1, 3000)), int(rng.integers(0, 500)), int(rng.integers(0, 40)), float(rng.choice([0.0, 5.0, 30.0])))


def test_native_check_against_the_reference(exe, tmp_path):
    rng = np.random.default_rng(20261021)
    cases = [_random_case(rng, k % 3) for k in range(90)]
    cases += [([], [], 1, 100, 20, 5.0), ([5, 5, 9], [0, 0, 3], 6, 100, 0, 0.0), ([5, 5], [7, 9], 6, 0, 0, 0.0)]        # no window; none with bases; none kept
    cases += [([5, 5], [1, 2], 0, 0, 1, 0.0), ([5, 5], [1, 2], 1, 500, 1, 0.0), ([5, 5], [1, 2], 1, 2 ** 63, 1, 0.0)]      # the refusals, through the file as well
    got = _run(exe, tmp_path, cases)
    assert got[-3:] == [None, None, None] and all(g is not None for g in got[:-3])
    exps = [ref.fit(*c) for c in cases[:-3]]
    for g, e in zip(got, exps):
        _same(g, e)
    assert {e["status"] for e in exps} == set(ref.STATUS)                   # every status is reached
    assert sum(e["status"] == "ok" for e in exps) >= 10 and any(e["n_f"] < e["n_kept"] - e["n_zero"] for e in exps) and any(e["n_fit"] < e["n_f"] for e in exps)


def test_planted_line_is_recovered(exe, tmp_path):
    """bases = round(len x 2^(a + b x)) at x = (rank + 0.5) / n: the fit returns b up to what the rounding of bases to an integer allows.  Rounding moves
    bases by at most 1/2, the depth by the relative d = 1 / (2 len depth), y = log2 depth by at most -log2(1 - d); a least-squares slope is
    sum(dx_j y_j) / sum(dx_j^2), so it moves by at most max|dy| x sum|dx_j| / sum(dx_j^2) (plus the f64 rounding of the sums, far below)."""
    rng = np.random.default_rng(7)
    n, a = 200, 5.0
    cases, bounds, slopes = [], [], []
    for b in (1.0, 0.25, 2.0):
        ln = rng.integers(2500, 5001, size=n)
        rank = rng.permutation(n)                                            # window i holds rank rank[i]
        x = (rank + 0.5) / n
        depth = 2.0 ** (a + b * x)
        bs = np.rint(ln * depth).astype(np.int64)
        cases.append((ln, bs, 2500, 0, 20, 5.0))
        dy = max(-math.log2(1.0 - 1.0 / (2.0 * float(l) * float(d))) for l, d in zip(ln, depth))
        xs = (np.arange(n) + 0.5) / n
        dx = xs - xs.mean()
        bounds.append(dy * np.abs(dx).sum() / (dx * dx).sum() + 1e-12)
        slopes.append(b)
        order = sorted(range(n), key=lambda i: (bs[i] * 1.0 / ln[i], i))     # the shape: the rounding has not swapped two ranks
        assert [int(rank[i]) for i in order] == list(range(n))
    got = _run(exe, tmp_path, cases)
    for g, b, bound in zip(got, slopes, bounds):
        slope, icpt, r2, index = (float.fromhex(v) for v in g[6:10])
        print("planted b = %g: slope %.15g, bound %.3g, off by %.3g" % (b, slope, bound, abs(slope - b)))
        assert g[10] == "ok" and int(g[3]) == n and bound < 1e-4
        assert abs(slope - b) <= bound
        assert abs(icpt - a) <= bound and r2 > 1.0 - 1e-6 and abs(index - 2.0 ** b) <= 2.0 ** b * math.log(2.0) * bound * 1.01


def test_permuted_windows_give_identical_bits(exe, tmp_path):
    rng = np.random.default_rng(99)
    ln, bs, *_ = _random_case(rng, 0)
    while len(ln) < 50:
        ln, bs, *_ = _random_case(rng, 0)
    ln[:6], bs[:6] = [10, 20, 30, 10, 20, 30], [50, 100, 150, 50, 100, 150]    # equal depths under different (bases, len): the tie rule has something to order
    cases = [(ln, bs, 10, 100, 5, 0.0)]
    for _ in range(5):
        pm = rng.permutation(len(ln))
        cases.append((ln[pm], bs[pm], 10, 100, 5, 0.0))
    got = _run(exe, tmp_path, cases)
    assert got[0][10] == "ok" and all(g == got[0] for g in got[1:])          # the printed hexadecimal floats: every bit


def test_engine_growth_fit_mirrors_the_helper():
    from pantax_amd import engine
    rng = np.random.default_rng(5)
    for k in range(12):
        c = _random_case(rng, k % 3)
        got, exp = engine.growth_fit(*c), ref.fit(*c)
        assert {k2: got[k2] for k2 in INTS} == {k2: exp[k2] for k2 in INTS} and got["status"] == exp["status"]
        for k2 in FLOATS:
            assert got[k2] == exp[k2] or abs(got[k2] - exp[k2]) <= REL * abs(exp[k2])
    assert engine.growth_fit([], [], 1)["status"] == "empty" and engine.GROWTH_STATUS == ref.STATUS
    for bad in (dict(min_own=0), dict(min_own=1, trim_permille=500)):
        with pytest.raises(ValueError):
            engine.growth_fit([5, 5], [1, 2], **bad)
    with pytest.raises(ValueError):
        engine.growth_fit([5, 5], [1], 1)
