"""tests/bootstrap_ref.py (the numpy restatement of the bootstrap of the strain fit) pinned on a case computed by hand, and the library's two host
helpers -- pantax_hip_bootstrap_weight, pantax_hip_bootstrap_summary -- against it.  No GPU: the helpers take no ctx."""
import math

import numpy as np

from tests import bootstrap_ref as ref


def _lib():
    from pantax_amd import _ffi
    return _ffi.load()


# ---- the hand case: one species (key 562, seed 42), 3 selected strains, 8 nodes
NODE_LEN = [10, 4, 5, 8, 2, 6, 3, 7]
BASES = [20, 0, 15, 8, 7, 12, 9, 0]
MEMBER = [[1, 1, 0], [1, 0, 0], [0, 0, 0], [0, 0, 1], [1, 0, 1], [0, 1, 0], [1, 1, 1], [0, 1, 0]]
# node 1 and node 7 have no coverage, node 2 no selected strain: five rows, in node order
ROWS_V = [0, 3, 4, 5, 6]
ROWS_MASK = [3, 4, 5, 2, 7]
ROWS_A = [2.0, 1.0, 3.5, 2.0, 3.0]
# sm(562) = 0x583afb6005b2b82f; sm(42 ^ sm(562)) = 0x26cb153f4791da56; r of replicate 1, nodes 0 .. 7, and the cell of the table it falls into
R1 = [0x1f5a21e79d066317, 0x5e48a89335777428, 0xc05a7c05d1d63b50, 0xcc03070513c0c614, 0x6cb514a92f8540b2, 0x8e909c39da156f60, 0xa85f6a9b85ac1757, 0xed8d1ac39668e39c]
W1 = [0, 1, 2, 2, 1, 1, 1, 3]
W2 = [2, 1, 1, 0, 0, 0, 1, 0]


def test_poisson_table_is_the_distribution_function():
    T = ref.T
    assert len(T) == 16 and all(T[j] < T[j + 1] for j in range(15)) and T[15] < 1 << 64
    assert T[0] == 0x5E2D58D8B3BCDF1A and T[1] == 2 * T[0] + 1              # e^-1 and 2 e^-1, floored: 6787... / 2^64; the halves' fractions add up to one more
    for j in range(16):
        exact = sum(math.exp(-1) / math.factorial(i) for i in range(j + 1))
        assert abs(T[j] / 2.0 ** 64 - exact) < 1e-15


def test_hand_case_rows_weights_and_expansion():
    member = np.array(MEMBER, dtype=bool)
    mask, a, v = ref.species_rows(NODE_LEN, BASES, member)
    assert v.tolist() == ROWS_V and mask.tolist() == ROWS_MASK and a.tolist() == ROWS_A
    assert ref.sm(562) == 0x583afb6005b2b82f and ref.sm(42 ^ ref.sm(562)) == 0x26cb153f4791da56
    h = 0x26cb153f4791da56
    assert [ref.sm((h + (1 << 40) + n) & ref.M64) for n in range(8)] == R1
    # T[0] = 0x5E2D.., T[1] = 0xBC5A.., T[2] = 0xEB71.., T[3] = 0xFB23..: 0x1f5a < T[0] -> 0; 0x5e48 >= T[0] -> 1; 0xc05a, 0xcc03 >= T[1] -> 2; 0xed8d >= T[2] -> 3
    assert [ref.weight(42, 562, 1, n) for n in range(8)] == W1 and [ref.weight(42, 562, 2, n) for n in range(8)] == W2
    assert [ref.weight(42, 562, 0, n) for n in range(8)] == [1] * 8
    for b, w in ((1, W1), (2, W2)):
        assert ref.weights(42, 562, b, np.arange(8)).tolist() == w
    # replicate 1: the rows of nodes 0, 3, 4, 5, 6 drew 0, 2, 1, 1, 1 -- pattern 3 does not exist in it
    m1, a1 = ref.expand(mask, a, ref.weights(42, 562, 1, v))
    assert m1.tolist() == [2, 4, 4, 5, 7] and a1.tolist() == [2.0, 1.0, 1.0, 3.5, 3.0]
    # replicate 2: 2, 0, 0, 0, 1
    m2, a2 = ref.expand(mask, a, ref.weights(42, 562, 2, v))
    assert m2.tolist() == [3, 3, 7] and a2.tolist() == [2.0, 2.0, 3.0]
    m0, a0 = ref.expand(mask, a, ref.weights(42, 562, 0, v))
    assert m0.tolist() == [2, 3, 4, 5, 7] and a0.tolist() == [2.0, 2.0, 1.0, 3.5, 3.0]


def test_library_weight_equals_the_reference():
    from pantax_amd import engine
    lib = _lib()
    assert [lib.pantax_hip_bootstrap_weight(42, 562, 1, n) for n in range(8)] == W1
    assert [engine.bootstrap_weight(42, 562, 2, n) for n in range(8)] == W2
    rng = np.random.default_rng(31)
    seeds = rng.integers(0, 1 << 64, 10000, dtype=np.uint64)
    keys = rng.integers(0, 1 << 64, 10000, dtype=np.uint64)
    keys[:100] = rng.integers(0, 5000, 100)                                   # taxid-sized keys too
    reps = rng.integers(0, 1 << 32, 10000, dtype=np.uint64)
    reps[:500] = rng.integers(0, 3, 500)                                      # replicate 0 among them
    vs = rng.integers(0, 1 << 33, 10000, dtype=np.uint64)
    for s, k, b, v in zip(seeds.tolist(), keys.tolist(), reps.tolist(), vs.tolist()):
        assert lib.pantax_hip_bootstrap_weight(s, k, b, v) == ref.weight(s, k, b, v), (s, k, b, v)


def test_weight_histogram_is_poisson_one():
    """10^6 draws (1 000 replicates of 1 000 nodes): the count of cell j is Binomial(n, p_j), p_j = e^-1 / j! (cell 16: the tail, 1.9e-14) -- every cell
    within 4 standard deviations sqrt(n p (1 - p)) of n p.  The bound is the binomial's, not a measurement."""
    n = 0
    hist = np.zeros(17, dtype=np.int64)
    v = np.arange(1000, dtype=np.uint64)
    for b in range(1, 1001):
        w = ref.weights(7, 1280, b, v)
        hist += np.bincount(w, minlength=17)
        n += len(w)
    assert n == 10 ** 6 and hist.sum() == n
    p = [math.exp(-1) / math.factorial(j) for j in range(16)]
    p.append(max(0.0, 1.0 - sum(p)))
    for j in range(17):
        sd = math.sqrt(n * p[j] * (1 - p[j]))
        print(j, hist[j], n * p[j], sd)
        assert abs(hist[j] - n * p[j]) <= 4 * sd + 1e-9, j


def _summary_lib(x, status):
    from pantax_amd import engine
    return engine.bootstrap_summary(x, status)


def test_summary_equals_the_reference_bit_for_bit():
    rng = np.random.default_rng(5)
    ties = np.round(rng.uniform(0, 3, 100), 1)                                # 100 values on a grid of 31: ties, zeros among them
    ties[::7] = 0.0
    mixed_x = rng.uniform(0, 10, 40)
    mixed_st = np.where(rng.random(40) < 0.3, -5, 0).astype(np.int32)
    mixed_st[3] = 1
    cases = [(np.zeros(0), None), (np.array([2.5]), None), (np.array([1.0, 4.0]), None), (ties, None), (ties, np.zeros(100, dtype=np.int32)),
             (mixed_x, mixed_st), (mixed_x, np.full(40, -5, dtype=np.int32)), (np.array([0.1, 0.2, 0.3]), np.array([0, -5, -5], dtype=np.int32))]
    for x, st in cases:
        got, exp = _summary_lib(x, st), ref.summary(x, st)
        assert got.dtype == exp.dtype == np.float64 and got.tobytes() == exp.tobytes(), (x, st, got, exp)
    # the definitions on values one can check by eye
    s = ref.summary(np.array([1.0, 4.0]))
    assert s.tolist() == [2.0, 2.5, math.sqrt(4.5), 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0]   # floor(p * 1 / 1000) = 0 for every p < 1000
    s = ref.summary(np.array([2.5]))
    assert s.tolist() == [1.0, 2.5, 0.0, 2.5, 2.5, 2.5, 2.5, 2.5, 0.0, 2.5]
    assert ref.summary(np.zeros(0)).tolist() == [0.0] * 10
    s = ref.summary(np.arange(101, dtype=np.float64)[::-1])
    assert s[3:8].tolist() == [2.0, 25.0, 50.0, 75.0, 97.0] and s[8] == 1 / 101 and s[9] == 0.0   # floor(25 * 100 / 1000) = 2, .., floor(975 * 100 / 1000) = 97
    s = ref.summary(np.array([5.0, 1.0, 3.0]), np.array([0, 1, 0]))
    assert s[0] == 2 and s[1] == 4.0 and s[9] == 3.0
