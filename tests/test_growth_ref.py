"""tests/growth_ref.py -- the restatement of pantax_hip_strain_growth and pantax_hip_growth_fit that the GPU tests and the native check compare with --
pinned on cases done by hand: a node walked twice, a node longer than the window (empty windows), a species with one selected haplotype (every step is
own), two haplotypes with identical walks (nothing is own); and the fit on windows whose line can be read off."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import growth_ref as ref
from tests.cov_track_ref import track


def _graph(node_len, walks):
    off = np.concatenate([[0], np.cumsum([len(w) for w in walks])]).astype(np.uint64)
    return SimpleNamespace(node_len=np.array(node_len, dtype=np.uint32), path_off=off, path_nodes=np.array(sum(walks, []), dtype=np.uint32), n_paths=len(walks))


#            node 0  1  2   3  4
G0 = _graph([3, 5, 2, 12, 4], [[0, 1, 2, 1, 3], [0, 3, 4], [0, 1, 2, 1, 3]])   # haplotype 0 walks node 1 twice; haplotype 2 walks what haplotype 0 walks
BASES = np.array([30, 50, 20, 120, 8], dtype=np.uint64)


def _is(got, win_off, n_own, ln, len_own, bases_own):
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and all(g.dtype == np.uint64 for g in got[2:])
    assert [g.tolist() for g in got] == [win_off, n_own, ln, len_own, bases_own]


def test_two_haplotypes_window_4():
    """W = 4.  Haplotype 0: offsets 0, 3, 8, 10, 15 -> windows 0, 0, 2, 2, 3 of ceil(27 / 4) = 7; node 3 (12 bases) runs through windows 4 .. 6 and node 1
    through window 1, which stay empty.  Nodes 0 and 3 are shared with haplotype 1; node 1 is own at both visits.  Haplotype 1: offsets 0, 3, 15 ->
    windows 0, 0, 3 of 5; only node 4 is its own."""
    got = ref.windows([G0], [0, 2], [0, 1], 4, BASES)
    _is(got, [0, 7, 12], [1, 0, 2, 0, 0, 0, 0] + [0, 0, 0, 1, 0], [8, 0, 7, 12, 0, 0, 0] + [15, 0, 0, 4, 0], [5, 0, 7, 0, 0, 0, 0] + [0, 0, 0, 4, 0],
        [50, 0, 70, 0, 0, 0, 0] + [0, 0, 0, 8, 0])
    swapped = ref.windows([G0], [0, 2], [1, 0], 4, BASES)                      # the order of the selection moves the entries and nothing else
    _is(swapped, [0, 5, 12], [0, 0, 0, 1, 0] + [1, 0, 2, 0, 0, 0, 0], [15, 0, 0, 4, 0] + [8, 0, 7, 12, 0, 0, 0], [0, 0, 0, 4, 0] + [5, 0, 7, 0, 0, 0, 0],
        [0, 0, 0, 8, 0] + [50, 0, 70, 0, 0, 0, 0])


def test_one_selected_haplotype_owns_every_step():
    got = ref.windows([G0], [0, 1], [0], 4, BASES)
    _is(got, [0, 7], [2, 0, 2, 1, 0, 0, 0], [8, 0, 7, 12, 0, 0, 0], [8, 0, 7, 12, 0, 0, 0], [80, 0, 70, 120, 0, 0, 0])
    tr = track([G0], [0, 1], [0], 4, np.zeros(5, dtype=np.uint64), BASES)     # ... and the windows are the coverage track's
    assert np.array_equal(got[1], tr[1]) and np.array_equal(got[3], tr[2]) and np.array_equal(got[4], tr[4]) and np.array_equal(got[2], tr[2])


def test_identical_walks_own_nothing():
    got = ref.windows([G0], [0, 2], [0, 2], 4, BASES)
    _is(got, [0, 7, 14], [0] * 14, [8, 0, 7, 12, 0, 0, 0] * 2, [0] * 14, [0] * 14)


def test_one_window_and_two_species():
    """W beyond every genome: one window a strain; a second species keeps its own membership (its haplotype 0 is alone)"""
    g1 = _graph([7, 1], [[1, 0, 1]])
    got = ref.windows([G0, g1], [0, 2, 3], [0, 1, 0], 10 ** 9, np.concatenate([BASES, np.array([70, 9], dtype=np.uint64)]))
    _is(got, [0, 1, 2, 3], [3, 1, 3], [27, 19, 9], [12, 4, 9], [120, 8, 88])
    none = ref.windows([G0, g1], [0, 0, 0], [], 4, np.zeros(7, dtype=np.uint64))
    assert none[0].tolist() == [0] and all(len(x) == 0 for x in none[1:])


def test_fit_by_hand():
    """depths 4, 1, 2, (0), and a window of 4 own bases that min_own = 5 drops: ranks 1 < 2 < 4 at x = 1/6, 3/6, 5/6, y = 0, 1, 2 -> slope 3, intercept -1/2"""
    r = ref.fit([10, 10, 10, 10, 4], [40, 10, 20, 0, 400], 5, 0, 2, 1.0)
    assert (r["n_kept"], r["n_zero"], r["n_f"], r["n_fit"], r["own_len"], r["status"]) == (4, 1, 3, 3, 40, "ok")
    assert r["median_depth"] == 2.0
    assert r["slope"] == pytest.approx(3.0, rel=1e-14) and r["intercept"] == pytest.approx(-0.5, rel=1e-13) and r["r2"] == pytest.approx(1.0, rel=1e-14)
    assert r["index"] == pytest.approx(8.0, rel=1e-13)
    assert ref.fit([10, 10, 10, 10, 4], [40, 10, 20, 0, 400], 5, 0, 4, 1.0)["status"] == "few_windows"
    assert ref.fit([10, 10, 10, 10, 4], [40, 10, 20, 0, 400], 5, 0, 4, 3.0)["status"] == "few_windows"      # the first that applies
    assert ref.fit([10, 10, 10, 10, 4], [40, 10, 20, 0, 400], 5, 0, 3, 3.0)["status"] == "low_depth"
    with_it = ref.fit([10, 10, 10, 10, 4], [40, 10, 20, 0, 400], 4, 0, 2, 1.0)                              # min_own = 4 keeps the window of depth 100: outside 8 x median
    assert (with_it["n_kept"], with_it["n_f"], with_it["own_len"], with_it["median_depth"]) == (5, 3, 44, 2.0) and with_it["slope"] == r["slope"]


def test_fit_order_median_trim():
    # equal depths as rationals (2/1 = 4/2 = 6/3) are one depth: flat, whatever their order
    r = ref.fit([1, 2, 3], [2, 4, 6], 1, 0, 1, 0.0)
    assert (r["status"], r["slope"], r["r2"], r["index"], r["intercept"], r["median_depth"]) == ("flat", 0.0, 0.0, 1.0, 1.0, 2.0)
    # the lower median of an even number; 1 000 is outside [1/8, 8] x 2 = the median, 16 is its upper edge and stays
    r = ref.fit([1] * 4, [1, 2, 16, 1000], 1, 0, 1, 0.0)
    assert (r["median_depth"], r["n_f"], r["n_fit"]) == (2.0, 3, 3)
    # ten windows of depth 2^0 .. 2^9 around the median 2^4: 2^0 (below 2) and 2^8, 2^9 (above 128) leave, n_f = 7; 150 thousandths trim floor(1.05) = 1
    # from each end: y = 2 .. 6 at x = (1.5 .. 5.5) / 7: slope 7
    r = ref.fit([1] * 10, [2 ** k for k in range(10)], 1, 150, 1, 0.0)
    assert (r["n_kept"], r["n_f"], r["n_fit"], r["median_depth"]) == (10, 7, 5, 16.0)
    assert r["slope"] == pytest.approx(7.0, rel=1e-13) and r["index"] == pytest.approx(128.0, rel=1e-12) and r["intercept"] == pytest.approx(2.0 - 1.5, rel=1e-12)
    rev = ref.fit([1] * 10, [2 ** k for k in range(9, -1, -1)], 1, 150, 1, 0.0)                             # the order of the windows does not enter
    assert rev == r
    # the order is exact where f64 is not: 2^60 + 1 over 2^60 against 1 over 1
    big = ref.fit([2 ** 60, 1, 1], [2 ** 60 + 1, 1, 2], 1, 0, 1, 0.0)
    assert big["n_fit"] == 3 and big["median_depth"] == 1.0                   # sorted 1/1 < (2^60 + 1)/2^60 < 2/1: the lower median is the middle one, 1.0 in f64
    assert ref.fit([5, 5], [0, 0], 1, 0, 1, 0.0)["status"] == "empty" and ref.fit([], [], 1)["status"] == "empty"
    e = ref.fit([5, 5], [0, 0], 1, 0, 1, 0.0)
    assert (e["n_kept"], e["n_zero"], e["n_f"], e["n_fit"], e["own_len"], e["median_depth"], e["slope"], e["index"]) == (2, 2, 0, 0, 10, 0.0, 0.0, 1.0)
    assert ref.min_own_of(5000) == 2500 and ref.min_own_of(1) == 1 and ref.min_own_of(100, 1000) == 100
