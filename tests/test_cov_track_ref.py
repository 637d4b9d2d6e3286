"""Pins the numpy restatement of the coverage-track contract (tests/cov_track_ref.py) on a micro case computed by hand, so that the GPU tests,
which compare the library with it, cannot agree with a wrong reading of the contract."""
import numpy as np

from tests.cov_track_ref import track, walk_windows

# five nodes; the walk visits node 1 twice and node 3 is longer than the window
NODE_LEN = np.array([3, 4, 2, 12, 5])
COV = np.array([3, 2, 0, 10, 1])
BASES = np.array([30, 8, 0, 100, 1])
WALK = [0, 1, 2, 1, 3, 4, 2]


def test_micro_walk_last_window_short():
    # W = 5.  offsets 0 3 7 9 13 25 30, G = 32 -> 7 windows; windows of the steps: 0 0 1 1 2 5 6
    # window 2 holds the 12-base node (13..24) alone, windows 3 and 4 see no node start, the last window holds 2 of its 5 bases
    n, ln, cv, bs = walk_windows(WALK, NODE_LEN, COV, BASES, 5)
    assert n.dtype == np.uint32 and ln.dtype == cv.dtype == bs.dtype == np.uint64
    assert n.tolist() == [2, 2, 1, 0, 0, 1, 1]
    assert ln.tolist() == [7, 6, 12, 0, 0, 5, 2]
    assert cv.tolist() == [5, 2, 10, 0, 0, 1, 0]
    assert bs.tolist() == [38, 8, 100, 0, 0, 1, 0]
    assert int(ln.sum()) == 32


def test_micro_walk_length_multiple_of_window():
    # W = 8: G = 32 = 4 W -> exactly 4 windows (no fifth, empty one).  windows of the steps: 0 0 0 1 1 3 3
    n, ln, cv, bs = walk_windows(WALK, NODE_LEN, COV, BASES, 8)
    assert n.tolist() == [3, 2, 0, 2]
    assert ln.tolist() == [9, 16, 0, 7]
    assert cv.tolist() == [5, 12, 0, 1]
    assert bs.tolist() == [38, 108, 0, 1]


def test_micro_walk_window_of_one_base_and_one_window():
    n, ln, cv, bs = walk_windows(WALK, NODE_LEN, COV, BASES, 1)
    starts = [0, 3, 7, 9, 13, 25, 30]
    assert len(n) == 32 and np.nonzero(n)[0].tolist() == starts and n.sum() == 7
    assert ln[starts].tolist() == [3, 4, 2, 4, 12, 5, 2] and bs[starts].tolist() == [30, 8, 0, 8, 100, 1, 0]
    n, ln, cv, bs = walk_windows(WALK, NODE_LEN, COV, BASES, 10 ** 9)
    assert (n.tolist(), ln.tolist(), cv.tolist(), bs.tolist()) == ([7], [32], [18], [147])
    assert all(len(a) == 0 for a in walk_windows([], NODE_LEN, COV, BASES, 5))


def test_micro_selection_order_and_offsets():
    class G:
        def __init__(self, node_len, walks):
            self.node_len = np.array(node_len)
            self.path_off = np.concatenate([[0], np.cumsum([len(w) for w in walks])]).astype(np.uint64)
            self.path_nodes = np.array([v for w in walks for v in w], dtype=np.uint32)
    species = [G([3, 4], [[0, 1], [1]]), G(NODE_LEN[:], [WALK, [4]])]
    cov = np.concatenate([[1, 2], COV])
    bases = np.concatenate([[5, 6], BASES])
    # species 0: haplotypes 1 then 0; species 1: haplotype 0 (node ids shifted by the two nodes of species 0)
    win_off, n, ln, cv, bs = track(species, [0, 2, 3], [1, 0, 0], 5, cov, bases)
    assert win_off.tolist() == [0, 1, 3, 10]
    # haplotype 1 of species 0: one node of 4 bases, one window; haplotype 0: 7 bases, two windows, both nodes start in the first
    assert n.tolist() == [1, 2, 0, 2, 2, 1, 0, 0, 1, 1]
    assert ln.tolist() == [4, 7, 0, 7, 6, 12, 0, 0, 5, 2]
    assert cv.tolist() == [2, 3, 0, 5, 2, 10, 0, 0, 1, 0]
    assert bs.tolist() == [6, 11, 0, 38, 8, 100, 0, 0, 1, 0]
