"""The LAD solver takes the same pivots as when tests/golden/lad_pivots.npz was recorded (tools/record_lad_pivots.py, on the commit before the solver's
body was split into phases): x as raw bit patterns, status and iterations of every case of tests/lad_pivot_cases.py -- under lad_shape=roomy, under
compact and at the default, one batch call per group -- and the tables and stats of the resident step of STEP_SET (both solves in lad_pair_kernel)."""
import os

import numpy as np
import pytest

from tests import lad_pivot_cases as lc
from tests.test_gpu_lad_shapes import _same


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return np.load(os.path.join(golden_dir, lc.GOLDEN))


@pytest.fixture(scope="module")
def cases(golden_dir):
    """group -> [(name, lp)]: made once, shared, never changed"""
    return lc.all_cases(golden_dir)


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def test_generated_cases_are_solved(cases, recorded):
    """CPU only: the oracle solves every generated LP, the record holds every case of every group with status 0, and every instance family pivoted"""
    from oracle import oracle as orc
    for group, lps in lc.generated_cases().items():
        for name, lp in lps:
            ub = np.where(lp["fixed"] == 1, 0.0, 1.05 * lp["a"].max())
            assert orc.lad_solve(lp["mask"], lp["a"], lp["p"], ub)[3] == 0, (group, name)
    assert max(lp["p"] for g in ("crafted16", "golden16") for _, lp in cases[g]) <= 16
    assert all(16 < lp["p"] <= 64 for g in ("cols64", "golden64") for _, lp in cases[g])
    assert all(64 < lp["p"] <= 256 for _, lp in cases["golden_wide"]) and all(lp["p"] > 256 for _, lp in cases["golden_huge"])
    assert sorted(lp["p"] for _, lp in cases["mixed"]) == [10, 17, 65, 257]
    pivoted = {}
    for group in lc.GROUPS:
        assert [n for n, _ in cases[group]] == recorded[group + "/names"].tolist(), group
        assert len(cases[group]) > 0 and np.all(recorded[group + "/status"] == 0), group
        assert recorded[group + "/x_off"][-1] == sum(lp["p"] for _, lp in cases[group]) == len(recorded[group + "/x_bits"]), group
        if group in lc.FAMILY:
            pivoted[lc.FAMILY[group]] = max(pivoted.get(lc.FAMILY[group], 0), int(recorded[group + "/iters"].max()))
    assert set(pivoted) == {"16", "64", "wide", "huge"} and min(pivoted.values()) > 3, pivoted


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [None, "roomy", "compact"])
@pytest.mark.parametrize("group", lc.GROUPS)
def test_same_pivots_as_recorded(eng, set_opt, cases, recorded, group, shape):
    set_opt(eng, "lad_shape", shape)
    got = lc.solve_group(eng, cases[group])
    names = [n for n, _ in cases[group]]
    print(group, shape, "iterations", got["iters"].tolist())
    assert np.array_equal(got["status"], recorded[group + "/status"]), (names, got["status"])
    assert np.array_equal(got["iters"], recorded[group + "/iters"]), (names, got["iters"], recorded[group + "/iters"])
    off = got["x_off"]
    assert np.array_equal(off, recorded[group + "/x_off"])
    for i, n in enumerate(names):
        assert np.array_equal(got["x_bits"][off[i]:off[i + 1]], recorded[group + "/x_bits"][off[i]:off[i + 1]]), n
    assert np.array_equal(got["obj"].view(np.uint64), recorded[group + "/obj"].view(np.uint64))   # summed from x outside the solver: the same bits too


@pytest.mark.gpu
def test_resident_step_as_recorded(eng, recorded):
    want = lc.from_json(str(recorded["step/json"]))
    got = lc.from_json(lc.to_json(lc.run_step(eng)))        # through the same text form: tuples and lists, arrays and their dtypes compare alike
    assert max(max(i) for i in got[2]["iters"]) > 3           # the LPs pivoted
    assert _same(got, want)
