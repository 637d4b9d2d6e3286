"""tests/addin_ref.py (the reference of the add-one test of the strain fit) checked without a GPU: every entry's objective against SciPy's HiGHS on the same
LP to 1e-9 relative -- on a random species and on the crafted species of tests/test_gpu_addin.py with hand-written depths --, the counts on a case computed
by hand, the stated answers of the crafted situations (asked here of the reference first, then of the device in the GPU test), the index arithmetic, and the
library's host helper pantax_hip_addin_donor against the restatement.  The helper takes no ctx."""
import numpy as np
import pytest

from tests import addin_ref as ref


def _random_species(seed, W, V, depth):
    rng = np.random.default_rng(seed)
    member = rng.random((V, W)) < 0.5
    node_len = rng.integers(20, 60, V)
    a_true = member.astype(np.float64) @ np.asarray(depth, dtype=np.float64)
    bases = rng.poisson(a_true * node_len)
    return node_len, bases, member


def _against_highs(d, K, J):
    for e in range(J + 1):
        ub = ref.box(d["a"], K, J, e)
        assert d["obj"][e] == pytest.approx(ref.highs_objective(d["mask"], d["a"], K + J, ub), rel=1e-9, abs=1e-12), e
        assert ref.residuals(d["mask"], d["a"], d["x"][e]).sum() == pytest.approx(d["obj"][e], rel=1e-12), e
        pinned = [K + c for c in range(J) if c + 1 != e]
        assert not d["x"][e][pinned].any() and np.all(d["x"][e] >= 0) and np.all(d["x"][e] <= 1.05 * d["a"].max())
    assert np.all(d["obj"][1:] <= d["obj"][0] * (1 + 1e-9))


def test_entries_against_highs():
    K, J = 3, 3
    # reported strains at 3x, 0 and 7.5x; candidate 0 absent, candidate 1 at 4x (a strain a filter dropped), candidate 2 at 1x
    node_len, bases, member = _random_species(51, K + J, 420, [3.0, 0.0, 7.5, 0.0, 4.0, 1.0])
    d = ref.species_addin(node_len, bases, member, K)
    assert d["rows"] >= 380 and np.all(d["status"] == 0) and np.all(np.diff(d["mask"].astype(np.int64)) >= 0)
    _against_highs(d, K, J)
    gain = d["obj"][0] - d["obj"][1:]
    # the dropped strain explains most of the misfit; the other two share half of its nodes and can take a little of its coverage, no more
    assert gain[1] > 0.5 * d["obj"][0] and gain[1] > 5 * max(gain[0], gain[2]) and min(gain) >= -1e-9 * d["obj"][0]
    assert d["x"][2][K + 1] == pytest.approx(4.0, rel=0.15)


def test_counts_by_hand():
    # K = 1, J = 2, six rows; x_base = (2, 0, 0); with candidate 0 free x_add = (1.5, 1, 0)
    mask = np.array([1, 1, 2, 3, 3, 6], dtype=np.uint64)
    a = np.array([2.0, 1.5, 1.0, 3.0, 2.5, 0.5])
    # predictions base: 2, 2, 0, 2, 2, 0 -> residuals 0, .5, 1, 1, .5, .5;   add: 1.5, 1.5, 1, 2.5, 2.5, 1 -> .5, 0, 0, .5, 0, .5
    assert ref.predictions(mask, [1.5, 1.0, 0.0]).tolist() == [1.5, 1.5, 1.0, 2.5, 2.5, 1.0]
    assert ref.counts(mask, a, 1, [2.0, 0.0, 0.0], [1.5, 1.0, 0.0], 0).tolist() == [4, 2, 4, 1]
    assert ref.counts(mask, a, 1, [2.0, 0.0, 0.0], [2.0, 0.0, 0.0], 1).tolist() == [1, 1, 0, 0]
    assert ref.counts0(mask, 1).tolist() == [6, 2, 0, 0] and ref.counts0(mask, 0).tolist() == [6, 6, 0, 0]
    assert ref.no_reported_bit(np.array([1 << 63], dtype=np.uint64), 64).tolist() == [False]
    # sel_off / cand_off of four species with (K, J) = (0, 0), (1, 1), (60, 4), (0, 64)
    so, co = [0, 0, 1, 61, 61], [0, 0, 1, 5, 69]
    assert ref.x_offsets(so, co).tolist() == [0, 0, 4, 4 + 5 * 64, 4 + 5 * 64 + 65 * 64]
    assert [ref.entry(co, s, e) for s, e in ((0, 0), (1, 1), (2, 4), (3, 64))] == [0, 2, 7, 72]


@pytest.mark.parametrize("name", sorted(ref.CRAFTED))
def test_crafted_species(name):
    case = ref.CRAFTED[name]
    K, J = len(case["sel"]), len(case["cand"])
    jitter = np.array([0.1 * ((i * 7) % 5 - 2) for i in range(case["n_nodes"])])
    node_len = np.full(case["n_nodes"], 10)
    bases = np.round((np.asarray(case["a"]) + jitter) * node_len).astype(np.int64)
    d = ref.species_addin(node_len, bases, ref.crafted_member(case), K)
    assert d["rows"] == case["n_nodes"] and np.all(d["status"] == 0)
    _against_highs(d, K, J)
    ref.assert_crafted("reference", name, d)
    if name == "dropped":
        c = case["cand"].index(1)
        j, loss, shift = ref.donor(K, d["x"][0], d["x"][c + 1])
        assert j == 0 and loss == pytest.approx(d["x"][0][0] - d["x"][c + 1][0]) and loss > 0 and shift == loss   # the one reported strain gives up what haplotype 1 takes
        assert d["x"][c + 1][K + c] == pytest.approx(8.0, abs=0.3) and d["x"][c + 1][0] == pytest.approx(5.0, abs=0.3)


def test_edges():
    node_len, bases, member = _random_species(53, 4, 50, [4.0, 2.0, 0.0, 1.0])
    # J = 0: entry 0 alone, the plain refit
    d = ref.species_addin(node_len, bases, member, 4)
    assert d["x"].shape == (1, 4) and d["status"].tolist() == [0] and d["count"][0].tolist() == [d["rows"], 0, 0, 0]
    _against_highs(d, 4, 0)
    # no column at all, and more than the call serves
    none = ref.species_addin(node_len, bases, np.zeros((50, 0), dtype=bool), 0)
    assert none["rows"] == 0 and none["status"].tolist() == [1] and none["x"].shape == (1, 0)
    wide = ref.species_addin(node_len, bases, np.ones((50, 65), dtype=bool), 60)
    assert wide["rows"] == 0 and np.all(wide["status"] == -4) and wide["x"].shape == (6, 65) and not wide["x"].any()


def test_donor_helper_mirrors_the_reference():
    from pantax_amd.engine import addin_donor
    rng = np.random.default_rng(54)
    cases = [(3, [1.0, 2.0, 3.0, 0.0], [0.5, 2.0, 2.0, 1.5]), (3, [1.0, 2.0, 3.0, 0.0], [0.5, 1.5, 3.0, 1.0]), (2, [1.0, 2.0, 0.0], [1.0, 2.5, 0.5]), (0, [0.0], [2.5]), (1, [2.0], [2.0])]
    for _ in range(50):
        W = int(rng.integers(1, 12))
        K = int(rng.integers(0, W + 1))
        cases.append((K, np.round(rng.random(W) * 4, 1), np.round(rng.random(W) * 4, 1)))   # a coarse grid: ties happen
    for K, xb, xa in cases:
        assert addin_donor(K, xb, xa) == ref.donor(K, xb, xa)
    assert addin_donor(3, [1.0, 2.0, 3.0, 0.0], [0.5, 2.0, 2.0, 1.5]) == (2, 1.0, 1.5)
    assert addin_donor(3, [1.0, 2.0, 3.0, 0.0], [0.5, 1.5, 3.0, 1.0]) == (0, 0.5, 1.0)       # a tie: the lowest column
    assert addin_donor(2, [1.0, 2.0, 0.0], [1.0, 2.5, 0.5]) == (-1, 0.0, 0.5)                 # no positive loss
    assert addin_donor(0, [0.0], [2.5]) == (-1, 0.0, 0.0)
    with pytest.raises(ValueError):
        addin_donor(3, [1.0, 2.0], [1.0, 0.0])
