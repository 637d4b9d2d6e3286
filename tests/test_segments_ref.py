"""tests/segments_ref.py -- the numpy restatement of pantax_hip_strain_segments and the plain-Python chain rule that the GPU tests compare against --
pinned on cases done by hand, and the host helper pantax_hip_segment_chain against the Python chain, element for element."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests.segments_ref import GAP, PEAK, chain, chain_arrays, segments, walk_runs

# eight nodes; the walk of haplotype 0 has twelve steps and visits the nodes 0, 4, 5 and 6 twice
NODE_LEN = np.array([10, 5, 20, 8, 3, 7, 12, 4], dtype=np.uint32)
COV = np.array([0, 0, 20, 8, 3, 0, 12, 4], dtype=np.uint32)
BASES = np.array([0, 0, 100, 8, 30, 0, 36, 4], dtype=np.uint64)       # depths 5, 1, 10, 3 (exactly), 1 on the covered nodes
WALK = [0, 1, 2, 4, 5, 4, 3, 6, 6, 7, 5, 0]
#  step      0   1   2   3   4   5   6   7   8   9  10  11
#  len      10   5  20   3   7   3   8  12  12   4   7  10
#  o_i       0  10  15  35  38  45  48  56  68  80  84  91      G = 101
#  class@3   g   g   p   p   g   p   0   p   p   0   g   g      (node 6: 36 >= 3 * 12 counts)
G0 = SimpleNamespace(node_len=NODE_LEN, path_off=np.array([0, 12, 14]), path_nodes=np.array(WALK + [2, 3]), n_paths=2)
SEL = (np.array([0, 1], dtype=np.uint64), np.array([0], dtype=np.uint32))

# class, step, n_steps, start, len, bases
A = (GAP, 0, 2, 0, 15, 0)         # a run at the walk's first step ...
B = (PEAK, 2, 2, 15, 23, 130)     # ... directly followed by a peak: two segments
C = (GAP, 4, 1, 38, 7, 0)
D = (PEAK, 5, 1, 45, 3, 30)
E = (PEAK, 7, 2, 56, 24, 72)      # node 6 twice: it counts at both visits
F = (GAP, 10, 2, 84, 17, 0)       # a run at the walk's last step


def _rows(r):
    return [tuple(int(a[i]) for a in r) for i in range(len(r[0]))]


def test_runs_by_hand():
    r = walk_runs(WALK, NODE_LEN, COV, BASES, 3)
    assert _rows(r) == [A, B, C, D, E, F]
    assert [a.dtype for a in r] == [np.uint8, np.uint64, np.uint32, np.uint64, np.uint64, np.uint64]
    assert _rows(walk_runs(WALK, NODE_LEN, COV, BASES, 4)) == [A, (PEAK, 2, 2, 15, 23, 130), C, D, F]      # node 6 at depth 3 is no peak at 4
    assert _rows(walk_runs(WALK, NODE_LEN, COV, BASES, 0)) == [A, C, F]                                    # peak_depth 0: no peak class
    assert _rows(walk_runs([], NODE_LEN, COV, BASES, 3)) == []
    assert _rows(walk_runs([2], NODE_LEN, COV, BASES, 6)) == []
    assert _rows(walk_runs([5], NODE_LEN, COV, BASES, 6)) == [(GAP, 0, 1, 0, 7, 0)]


@pytest.mark.parametrize("min_len,kept", [(1, [A, B, C, D, E, F]), (7, [A, B, C, E, F]), (8, [A, B, E, F]), (24, [E]), (25, [])])
def test_min_len_is_inclusive(min_len, kept):
    """len == min_len is kept, min_len + 1 drops it (C at 7 / 8, E at 24 / 25); the totals count every run whatever min_len is"""
    seg_off, hap_len, n_runs, run_len, run_max, *seg = segments([G0], *SEL, 3, min_len, COV, BASES)
    assert _rows(seg) == kept and seg_off.tolist() == [0, len(kept)]
    assert hap_len.tolist() == [101]
    assert n_runs.tolist() == [[3, 3]] and run_len.tolist() == [[39, 50]] and run_max.tolist() == [[17, 24]]


def test_selection_order_and_peak_depth_per_entry():
    sel = (np.array([0, 2], dtype=np.uint64), np.array([1, 0], dtype=np.uint32))
    seg_off, hap_len, n_runs, run_len, run_max, *seg = segments([G0], *sel, [5, 0], 1, COV, BASES)
    assert seg_off.tolist() == [0, 1, 4] and hap_len.tolist() == [28, 101]
    assert _rows(seg) == [(PEAK, 0, 1, 0, 20, 100), A, C, F]                  # haplotype 1 = nodes 2, 3 at depth 5 and 1; haplotype 0 without peaks
    assert n_runs.tolist() == [[0, 1], [3, 0]] and run_max.tolist() == [[0, 20], [17, 0]]
    assert segments([G0], np.array([0, 0], dtype=np.uint64), np.zeros(0, dtype=np.uint32), 3, 1, COV, BASES)[0].tolist() == [0]


# the chain rule: class, start, len, n_steps, bases
SEGS = [(GAP, 0, 10, 1, 0), (GAP, 20, 5, 2, 0), (PEAK, 25, 5, 1, 99), (GAP, 31, 4, 1, 0), (GAP, 46, 1, 1, 0)]


def _chain(segs, bridge, min_span):
    cols = list(zip(*segs)) if segs else [[]] * 5
    return chain(*cols, bridge, min_span)


def _brief(chains):
    return [(c["class"], c["start"], c["end"], c["in_class"], c["n_segments"], c["first"], c["last"]) for c in chains]


def test_chain_by_hand():
    # separation == bridge merges (10 -> 20), a peak between two gaps does not break their chain, bridge + 1 does not merge (35 -> 46)
    assert _brief(_chain(SEGS, 10, 0)) == [(GAP, 0, 35, 19, 3, 0, 3), (PEAK, 25, 30, 5, 1, 2, 2), (GAP, 46, 47, 1, 1, 4, 4)]
    assert _brief(_chain(SEGS, 9, 0)) == [(GAP, 0, 10, 10, 1, 0, 0), (GAP, 20, 35, 9, 2, 1, 3), (PEAK, 25, 30, 5, 1, 2, 2), (GAP, 46, 47, 1, 1, 4, 4)]
    assert _brief(_chain(SEGS, 11, 0)) == [(GAP, 0, 47, 20, 4, 0, 4), (PEAK, 25, 30, 5, 1, 2, 2)]
    c = _chain(SEGS, 10, 0)[0]
    assert c["span"] == 35 and c["n_steps"] == 4 and c["bases"] == 0
    # bridge = 0: only segments that touch
    assert _brief(_chain(SEGS, 0, 0)) == [(k, s, s + n, n, 1, i, i) for i, (k, s, n, _, _) in enumerate(SEGS)]
    assert _brief(_chain([(GAP, 0, 10, 1, 0), (GAP, 10, 5, 1, 0), (GAP, 16, 1, 1, 0)], 0, 0)) == [(GAP, 0, 15, 15, 2, 0, 1), (GAP, 16, 17, 1, 1, 2, 2)]
    # the span filter, inclusive, on the chain and not on its members
    assert _brief(_chain(SEGS, 10, 5)) == [(GAP, 0, 35, 19, 3, 0, 3), (PEAK, 25, 30, 5, 1, 2, 2)]
    assert _brief(_chain(SEGS, 10, 6)) == [(GAP, 0, 35, 19, 3, 0, 3)]
    assert _brief(_chain(SEGS, 10, 35)) == [(GAP, 0, 35, 19, 3, 0, 3)] and _chain(SEGS, 10, 36) == []
    assert _chain([], 10, 0) == []


def _random_table(rng):
    n = int(rng.integers(0, 40))
    gaps = rng.integers(0, 6, n) * rng.integers(0, 2, n)                     # many segments that touch
    lens = rng.integers(1, 30, n)
    start = np.cumsum(gaps + np.concatenate([[0], lens[:-1]])) if n else np.zeros(0, dtype=np.int64)
    return (rng.integers(1, 3, n).astype(np.uint8), start.astype(np.uint64), lens.astype(np.uint64), rng.integers(1, 9, n).astype(np.uint32),
            rng.integers(0, 2 ** 40, n).astype(np.uint64))


def test_host_helper_equals_the_reference():
    from pantax_amd import engine
    rng = np.random.default_rng(20261020)
    n_chains = 0
    for _ in range(300):
        t = _random_table(rng)
        bridge, min_span = int(rng.integers(0, 8)), int(rng.integers(0, 40))
        exp = chain_arrays(chain(*t, bridge, min_span))
        got = engine.segment_chain(*t, bridge, min_span)
        for a, b in zip(got, exp):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
        n_chains += len(exp[0])
    assert n_chains > 300
    got = engine.segment_chain(*zip(*SEGS), 10, 6)
    assert got[0].tolist() == [GAP] and got[3].tolist() == [[0, 35, 35, 19, 3, 4, 0]]
    big = engine.segment_chain([1, 1], [0, 2 ** 63], [5, 7], [1, 1], [2 ** 63, 2 ** 62], 2 ** 64 - 1, 0)   # a bridge over everything, u64 sums
    assert big[3].tolist() == [[0, 2 ** 63 + 7, 2 ** 63 + 7, 12, 2, 2, 2 ** 63 + 2 ** 62]]
    for bad in (([3], [0], [1], [1], [0]), ([0], [0], [1], [1], [0]),        # a class that is neither gap nor peak
                ([1, 1], [5, 0], [1, 1], [1, 1], [0, 0]),                    # not ascending
                ([1, 2], [0, 9], [10, 1], [1, 1], [0, 0]),                   # overlapping, whatever the classes
                ([1], [2 ** 64 - 1], [2], [1], [0])):                        # an end that wraps
        with pytest.raises(ValueError):
            engine.segment_chain(*bad, 0, 0)
