"""tests/dropout_ref.py (the reference of the leave-one-out test of the strain fit) checked on crafted species: every entry's objective against SciPy's
HiGHS on the same LP to 1e-9 relative, the counts on a case computed by hand, the stated answers of the three crafted situations (two strains with the
same walk, a strain with private nodes, a strain the refit puts at zero), and the library's host helper pantax_hip_dropout_substitute against the
restatement.  No GPU: the helper takes no ctx."""
import numpy as np
import pytest

from tests import dropout_ref as ref


def _random_species(seed, K, V, depth):
    rng = np.random.default_rng(seed)
    member = rng.random((V, K)) < 0.5
    node_len = rng.integers(20, 60, V)
    a_true = member.astype(np.float64) @ np.asarray(depth, dtype=np.float64)
    bases = rng.poisson(a_true * node_len)
    return node_len, bases, member


def test_entries_against_highs():
    K = 5
    node_len, bases, member = _random_species(41, K, 420, [3.0, 0.0, 7.5, 1.0, 4.0])
    d = ref.species_dropout(node_len, bases, member)
    assert d["rows"] >= 380 and np.all(d["status"] == 0) and np.all(np.diff(d["mask"].astype(np.int64)) >= 0)
    for e in (0, 1, 2, 5):                                                   # dropping none, column 0, column 1 and column 4
        ub = ref.box(d["a"], K, None if e == 0 else e - 1)
        assert d["obj"][e] == pytest.approx(ref.highs_objective(d["mask"], d["a"], K, ub), rel=1e-9)
        assert np.abs(ref.residuals(d["mask"], d["a"], d["x"][e])).sum() == pytest.approx(d["obj"][e], rel=1e-12)
        if e:
            assert d["x"][e][e - 1] == 0.0
    assert np.all(d["obj"][1:] >= d["obj"][0] * (1 - 1e-9))
    assert d["obj"][1] > 1.05 * d["obj"][0] and d["obj"][3] > 1.05 * d["obj"][0]   # the strains at 3x and 7.5x are needed
    assert d["obj"][2] <= d["obj"][0] * (1 + 1e-6) + 1e-9                    # the strain that is not there costs next to nothing to remove


def test_counts_by_hand():
    # K = 2, six rows; x_full = (2, 1), without column 0 x_drop = (0, 2.5)
    mask = np.array([1, 1, 2, 3, 3, 3], dtype=np.uint64)
    a = np.array([2.0, 2.5, 1.0, 3.0, 2.5, 1.0])
    # predictions full: 2, 2, 1, 3, 3, 3 -> residuals 0, .5, 0, 0, .5, 2;   drop: 0, 0, 2.5, 2.5, 2.5, 2.5 -> 2, 2.5, 1.5, .5, 0, 1.5
    assert ref.predictions(mask, [2.0, 1.0]).tolist() == [2.0, 2.0, 1.0, 3.0, 3.0, 3.0]
    assert ref.counts(mask, a, [2.0, 1.0], [0.0, 2.5], 0).tolist() == [5, 2, 4, 2]
    assert ref.counts(mask, a, [2.0, 1.0], [2.0, 1.0], 1).tolist() == [4, 1, 0, 0]
    assert ref.x_offsets([0, 0, 1, 65, 130]).tolist() == [0, 0, 2, 2 + 65 * 64, 2 + 65 * 64 + 66 * 65]
    assert [ref.entry([0, 0, 1, 65, 130], s, e) for s, e in ((0, 0), (1, 1), (2, 64), (3, 65))] == [0, 2, 67, 133]


def _walk_species(walks, n_nodes, a_of_node, node_len=10):
    member = np.zeros((n_nodes, len(walks)), dtype=bool)
    for k, w in enumerate(walks):
        member[w, k] = True
    return np.full(n_nodes, node_len), (np.asarray(a_of_node) * node_len).astype(np.int64), member


def test_two_strains_with_the_same_walk():
    """A vertex of the LP holds at most one of two equal columns, so the refit puts one twin at zero: dropping the other moves its coverage to the first (its
    substitute, gain = what it held); dropping the one at zero changes nothing and by the helper's rule has no substitute."""
    # strains 0 and 1 walk nodes 0 .. 19, strain 2 nodes 10 .. 29: the sample has about 4x on 0 .. 9, 6x on 10 .. 19, 2x on 20 .. 29
    walks = [list(range(20)), list(range(20)), list(range(10, 30))]
    jitter = [0.1 * ((i * 7) % 5 - 2) for i in range(30)]
    d = ref.species_dropout(*_walk_species(walks, 30, [c + j for c, j in zip([4.0] * 10 + [6.0] * 10 + [2.0] * 10, jitter)]))
    assert d["rows"] == 30 and np.all(d["status"] == 0) and d["obj"][0] > 1.0
    assert max(d["x"][0][0], d["x"][0][1]) > 3.0
    for k, other in ((0, 1), (1, 0)):
        assert d["obj"][k + 1] - d["obj"][0] <= 1e-9 * d["obj"][0]
        j, gain, shift = ref.substitute(k, d["x"][0], d["x"][k + 1])
        if d["x"][0][k] > 0.0:
            assert j == other and gain == pytest.approx(d["x"][0][k], rel=1e-9)
        else:
            assert j == -1 and d["x"][0][other] > 0.0
        assert d["count"][k + 1].tolist()[:2] == [20, 0]
    assert d["obj"][3] - d["obj"][0] > 10.0 and d["count"][3].tolist()[:2] == [20, 10]   # without strain 2 its ten private nodes alone cost about 2x each


def test_private_nodes_and_a_strain_at_zero():
    # strain 0 walks 0 .. 14 (5 private), strain 1 walks 5 .. 24, strain 2 walks 5 .. 14 and nothing in the sample speaks for it
    walks = [list(range(15)), list(range(5, 25)), list(range(5, 15))]
    d = ref.species_dropout(*_walk_species(walks, 25, [3.0] * 5 + [8.0] * 10 + [5.0] * 10))
    assert np.all(d["status"] == 0) and d["obj"][0] == pytest.approx(0.0, abs=1e-9)
    assert d["x"][0] == pytest.approx([3.0, 5.0, 0.0], abs=1e-9) and d["x"][0][2] == 0.0
    assert d["obj"][1] - d["obj"][0] > 0 and d["count"][1][1] == 5             # private covered nodes: needed
    assert d["obj"][3] - d["obj"][0] == 0.0 and d["count"][3].tolist() == [10, 0, 0, 0]   # at zero in the refit: nothing changes without it
    assert ref.substitute(2, d["x"][0], d["x"][3]) == (-1, 0.0, 0.0)


def test_one_strain():
    node_len, bases, member = _random_species(43, 1, 50, [4.0])
    d = ref.species_dropout(node_len, bases, member)
    assert d["x"].shape == (2, 1) and d["x"][1][0] == 0.0 and d["status"].tolist() == [0, 0]
    x0 = d["x"][0][0]
    assert d["obj"][1] == pytest.approx(d["a"].sum(), rel=1e-12) and x0 > 3.0
    # without the one column a row costs a instead of |x0 - a|: more for a > x0 / 2, less for a < x0 / 2
    assert d["count"][1].tolist() == [d["rows"], d["rows"], int((d["a"] > np.abs(x0 - d["a"])).sum()), int((d["a"] < np.abs(x0 - d["a"])).sum())]
    assert d["obj"][0] == pytest.approx(ref.highs_objective(d["mask"], d["a"], 1, ref.box(d["a"], 1)), rel=1e-9)
    # nothing selected, and more than the call serves
    none = ref.species_dropout(node_len, bases, np.zeros((50, 0), dtype=bool))
    assert none["rows"] == 0 and none["status"].tolist() == [1] and none["x"].shape == (1, 0)
    wide = ref.species_dropout(node_len, bases, np.ones((50, 65), dtype=bool))
    assert wide["rows"] == 0 and np.all(wide["status"] == -4) and wide["x"].shape == (66, 65) and not wide["x"].any()


def test_substitute_helper_mirrors_the_reference():
    from pantax_amd.engine import dropout_substitute
    rng = np.random.default_rng(44)
    cases = [([1.0, 2.0, 3.0, 4.0], [0.0, 2.5, 3.5, 4.25], 0), ([1.0, 2.0, 3.0, 4.0], [0.0, 1.5, 3.0, 3.0], 0), ([2.5], [0.0], 0), ([1.0, 2.0], [1.0, 2.0], 1)]
    for _ in range(50):
        K = int(rng.integers(1, 12))
        xf = np.round(rng.random(K) * 4, 1)                                   # a coarse grid: ties happen
        xd = np.round(rng.random(K) * 4, 1)
        k = int(rng.integers(0, K))
        xd[k] = 0.0
        cases.append((xf, xd, k))
    for xf, xd, k in cases:
        assert dropout_substitute(k, xf, xd) == ref.substitute(k, xf, xd)
    assert dropout_substitute(0, [1.0, 2.0, 3.0, 4.0], [0.0, 2.5, 3.5, 4.25]) == (1, 0.5, 1.25)
    with pytest.raises(ValueError):
        dropout_substitute(2, [1.0, 2.0], [1.0, 0.0])
