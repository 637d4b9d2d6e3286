"""Pins the plain-Python reading of the depth-distribution contract (tests/depth_ref.py) on hand-written tables and a micro case computed by hand, and
the host helpers of the library (pantax_hip_depth_bin / _bin_range / _quantile, called through ctypes: they need no GPU) against it -- so that the GPU
tests, which compare the kernel with depth_ref, cannot agree with a wrong reading of the contract.

One place where the contract cannot be taken literally: `lo(bin(d)) <= d < hi(bin(d))` with hi(95) = 2^64 - 1 excludes d = 2^64 - 1 itself, which is a
u64 depth and falls into bin 95.  The tests ask for the strict inequality everywhere else and for d <= hi(95) at that single value."""
import ctypes as C
import random

import numpy as np
import pytest

from tests import depth_ref as ref

U64_MAX = 2 ** 64 - 1
# d -> bin, written out by hand from the contract: exact below 32; [32, 40) [40, 48) [48, 56) [56, 64) are the four quarters of the octave of 2^5;
# 64 opens the octave of 2^6; 2^21 - 1 lies in the last quarter of the octave of 2^20 = 32 + 4 * 15 + 3; everything from 2^21 up stays in 95
BIN_TABLE = [(0, 0), (1, 1), (31, 31), (32, 32), (39, 32), (40, 33), (47, 33), (48, 34), (55, 34), (56, 35), (63, 35), (64, 36),
             (2 ** 21 - 1, 95), (2 ** 21, 95), (2 ** 40, 95), (U64_MAX, 95)]


def _random_depths():
    rng = random.Random(20261018)
    out = []
    for _ in range(10000):
        bits = rng.randint(1, 64)                  # every magnitude, not only the top octaves
        out.append(rng.getrandbits(bits))
    return out


def _in_range(d, lo, hi):
    return lo <= d < hi or (d == U64_MAX and hi == U64_MAX and lo <= d)


@pytest.fixture(scope="module")
def lib():
    from pantax_amd import _ffi
    return _ffi.load()


def _c_range(lib, b):
    lo, hi = C.c_uint64(0), C.c_uint64(0)
    rc = lib.pantax_hip_depth_bin_range(b, C.byref(lo), C.byref(hi))
    return rc, int(lo.value), int(hi.value)


def _c_quantile(lib, hist, pm, preset=1234):
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    assert h.shape == (ref.BINS, 2)
    out = C.c_uint32(preset)
    rc = lib.pantax_hip_depth_quantile(h.ctypes.data_as(C.c_void_p), pm, C.byref(out))
    return rc, int(out.value)


def test_bin_table():
    assert [ref.depth_bin(d) for d, _ in BIN_TABLE] == [b for _, b in BIN_TABLE]


def test_bin_ranges_hold_their_depths():
    for d in [d for d, _ in BIN_TABLE] + _random_depths():
        lo, hi = ref.bin_range(ref.depth_bin(d))
        assert _in_range(d, lo, hi), (d, lo, hi)


def test_bin_bounds_increase_and_tile():
    los = [ref.bin_range(b)[0] for b in range(ref.BINS)]
    assert all(a < b for a, b in zip(los, los[1:]))                              # lo is strictly increasing
    assert los[:33] == list(range(33)) and los[33:37] == [40, 48, 56, 64] and los[95] == 7 << 18
    assert all(ref.bin_range(b)[1] == los[b + 1] for b in range(ref.BINS - 1)) and ref.bin_range(95)[1] == U64_MAX   # hi(b) = lo(b + 1): no gap, no overlap
    assert all(ref.depth_bin(lo) == b for b, lo in enumerate(los))               # every lower bound opens its own bin ...
    assert all(ref.depth_bin(los[b] - 1) == b - 1 for b in range(1, ref.BINS))   # ... and the depth just below closes the one before


def _hist(entries):
    h = [[0, 0] for _ in range(ref.BINS)]
    for b, n, length in entries:
        h[b] = [n, length]
    return h


# three hand-made histograms: all length in one bin; two bins with a tie exactly at the target; no length at all
ONE_BIN = _hist([(40, 3, 77)])
TIE = _hist([(3, 1, 500), (50, 2, 500)])          # T = 1000: the target at p per mille is exactly p
NO_LEN = _hist([(0, 4, 0), (9, 1, 0)])            # nodes, but no base of length
QUANTILE_CASES = [(ONE_BIN, pm, 40) for pm in (0, 1, 50, 500, 999, 1000)] + \
                 [(TIE, 0, 3), (TIE, 1, 3), (TIE, 499, 3), (TIE, 500, 3),        # cumulative len 500 >= target 500: the tie goes to the lower bin
                  (TIE, 501, 50), (TIE, 950, 50), (TIE, 1000, 50)] + \
                 [(NO_LEN, pm, None) for pm in (0, 500, 1000)]


def test_quantile_by_hand():
    for hist, pm, want in QUANTILE_CASES:
        assert ref.quantile(hist, pm) == want, (pm, want)
    assert ref.quantile(_hist([(0, 1, 1), (95, 1, 1)]), 0) == 0                  # a target of 0 is raised to 1: the first bin with any length
    assert ref.quantile(_hist([(2, 5, 0), (7, 1, 3)]), 0) == 7                   # ... which skips bins that hold nodes without length


def test_c_helpers_equal_the_python(lib):
    from pantax_amd import engine
    from pantax_amd._ffi import DEPTH_BINS, DEPTH_NONE
    assert DEPTH_BINS == ref.BINS
    for d, b in BIN_TABLE:
        assert lib.pantax_hip_depth_bin(d) == b == engine.depth_bin(d)
    for d in _random_depths():
        b = lib.pantax_hip_depth_bin(d)
        assert b == ref.depth_bin(d), d
        rc, lo, hi = _c_range(lib, b)
        assert rc == 0 and _in_range(d, lo, hi)
    for b in range(ref.BINS):
        assert _c_range(lib, b) == (0,) + ref.bin_range(b) and engine.depth_bin_range(b) == ref.bin_range(b)
    assert _c_range(lib, ref.BINS)[0] == -1 and lib.pantax_hip_depth_bin_range(0, None, None) == -1     # PANTAX_HIP_E_INVALID
    with pytest.raises(ValueError):
        engine.depth_bin_range(ref.BINS)
    for hist, pm, want in QUANTILE_CASES:
        rc, out = _c_quantile(lib, hist, pm)
        if want is None:
            assert rc == DEPTH_NONE and out == 1234                              # "none", and the output is left alone
        else:
            assert (rc, out) == (0, want)
        assert engine.depth_quantile(hist, pm) == want
    rc, out = _c_quantile(lib, TIE, 1001)
    assert rc == -1 and out == 1234
    with pytest.raises(ValueError):
        engine.depth_quantile(TIE, 1001)
    big = _hist([(10, 1, U64_MAX), (20, 1, U64_MAX), (30, 1, U64_MAX)])          # T beyond u64: the sums must not wrap
    for pm, want in ((333, 10), (334, 20), (667, 30)):
        assert ref.quantile(big, pm) == want and _c_quantile(lib, big, pm) == (0, want)


# ---- five nodes, three haplotypes; the selection is haplotype 2, then haplotype 0 (haplotype 1 is in the db and not selected)
#   node   len   bases        depth   bin
#   0      10    35           3       3
#   1      4     0            0       0       walked twice by haplotype 0
#   2      100   4000         40      33
#   3      2     700          350     45      e = 8, (350 >> 6) & 3 = 1: 32 + 12 + 1; walked only by haplotype 1: an orphan
#   4      7     6            0       0       6 // 7 = 0
NODE_LEN = [10, 4, 100, 2, 7]
BASES = [35, 0, 4000, 700, 6]
WALKS = [[0, 1, 2, 1], [0, 3], [0, 2, 4]]
# M(0) = {2, 0}, M(1) = {0}, M(2) = {2, 0}, M(3) = {}, M(4) = {2}
H2_ALL = _hist([(3, 1, 10), (33, 1, 100), (0, 1, 7)])         # nodes 0 2 4
H2_PRIVATE = _hist([(0, 1, 7)])                               # node 4
H0_ALL = _hist([(3, 1, 10), (0, 1, 4), (33, 1, 100)])         # nodes 0 1 2, node 1 once
H0_PRIVATE = _hist([(0, 1, 4)])                               # node 1
TOTAL = _hist([(0, 2, 11), (3, 1, 10), (33, 1, 100), (45, 1, 2)])
ORPHAN = _hist([(45, 1, 2)])


def test_micro_case_all_four_classes():
    hap, sp = ref.species_depth(NODE_LEN, [WALKS[2], WALKS[0]], BASES)
    assert hap == [[H2_ALL, H2_PRIVATE], [H0_ALL, H0_PRIVATE]]
    assert sp == [TOTAL, ORPHAN]
    hap, sp = ref.species_depth(NODE_LEN, [], BASES)                             # nothing selected: every node is an orphan
    assert hap == [] and sp == [TOTAL, TOTAL]
    hap, sp = ref.species_depth([0, 5], [[0, 1]], [9, 4])                        # a node without bases of length has depth 0
    assert hap == [[_hist([(0, 2, 5)]), _hist([(0, 2, 5)])]] and sp == [_hist([(0, 2, 5)]), _hist([])]


def test_micro_case_db_offsets_and_rows():
    class G:
        def __init__(self, node_len, walks):
            self.node_len = np.array(node_len)
            self.path_off = np.concatenate([[0], np.cumsum([len(w) for w in walks])]).astype(np.uint64)
            self.path_nodes = np.array([v for w in walks for v in w], dtype=np.uint32)
    species = [G([3, 4], [[0, 1], [1]]), G(NODE_LEN, WALKS), G([9], [[0]])]
    bases = np.array([6, 400] + BASES + [90], dtype=np.uint64)
    # species 0: haplotype 1; species 1: haplotypes 2 then 0; species 2: nothing
    hap, sp = ref.depth(species, [0, 1, 3, 3], [1, 2, 0], np.zeros(8, dtype=np.uint32), bases)
    assert hap.dtype == sp.dtype == np.uint64 and hap.shape == (3, 2, 96, 2) and sp.shape == (3, 2, 96, 2)
    # species 0: node 0 (len 3, depth 2) is an orphan, node 1 (len 4, depth 100: e = 6, (100 >> 4) & 3 = 2, bin 38) is private to haplotype 1
    assert hap[0].tolist() == [_hist([(38, 1, 4)]), _hist([(38, 1, 4)])]
    assert hap[1].tolist() == [H2_ALL, H2_PRIVATE] and hap[2].tolist() == [H0_ALL, H0_PRIVATE]
    assert sp.tolist() == [[_hist([(2, 1, 3), (38, 1, 4)]), _hist([(2, 1, 3)])], [TOTAL, ORPHAN], [_hist([(10, 1, 9)]), _hist([(10, 1, 9)])]]
    # the rows of the report for species 1.  total: T = 123, cumulative len 11 (bin 0), 21 (bin 3), 121 (bin 33), 123 (bin 45); the targets are
    # ceil(6.15) = 7, ceil(30.75) = 31, 62, 93, 117 -> bins 0, 33, 33, 33, 33; lo(33) = 40, hi(33) = 48
    rows = ref.report_rows([("77", "770", "GCF_2", hap[1][0], hap[1][1], "12.5")], [("77", sp[1][0], sp[1][1])])
    assert rows == [ref.HEADER,
                    ["77", "770", "GCF_2", "all", "3", "117", "7", "0", "40", "40", "40", "40", "48", "12.5"],       # 7 | 17 | 117; targets 6 30 59 88 112
                    ["77", "770", "GCF_2", "private", "1", "7", "7", "0", "0", "0", "0", "0", "1", "12.5"],
                    ["77", "-", "-", "total", "5", "123", "11", "0", "40", "40", "40", "40", "48", "-"],
                    ["77", "-", "-", "orphan", "1", "2", "0", "320", "320", "320", "320", "320", "384", "-"]]       # bin 45 = [320, 384)
    assert ref.hist_row("1", "-", "-", "orphan", _hist([(0, 3, 0)]), "-") == ["1", "-", "-", "orphan", "3", "0", "0", "-", "-", "-", "-", "-", "-", "-"]
