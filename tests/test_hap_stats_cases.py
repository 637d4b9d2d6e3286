"""The crafted a9 cases of tests/hap_stats_cases.py, checked without a GPU: every case's conditions on its INPUTS hold in exact arithmetic (no |z| near
3, variance 0 or clearly positive, first-filter fractions exactly at or clear of their thresholds), the oracle agrees with the exact restatement, and
each case really is what its name says (the outlier is dropped at 13 values and kept at 9, the equal-valued haplotypes have sd == 0, the degenerate
ones split the sequential sum from the pairwise tree, ...)."""
from fractions import Fraction

import numpy as np
import pytest

from tests import hap_stats_cases as hc


@pytest.mark.parametrize("name", hc.CASE_NAMES)
def test_case_is_admitted(name):
    case = hc.get_case(name)
    bad = hc.admit(case)
    assert not bad, "\n".join(bad)
    assert case.reads.n_reads <= 6000 and case.reference()["keep"].sum() == len(case.species) - len(case.dropped)


def test_generator_steers_every_window():
    """the plan's n * bases arrive in the oracle's trio_bases of exactly that window, and nothing else of the table is touched"""
    g = hc.crafted_species("1", 5, 8, 1)
    plan = {0: {0: (2, 102), 7: (1, 300)}, 3: {4: (3, 201)}, 4: {1: (1, 150), 2: (1, 150)}}
    case = hc.Case("probe", [g], [hc.window_reads(g, plan)])
    T, tb = case.reference()["species"][0]["T"], case.reference()["species"][0]["tb"]
    assert T.n_unique == 5 * 8 and np.all(T.len == hc.WIN_LEN) and np.all(np.diff(T.hap_off) == 8)
    want = np.zeros(T.n_unique, dtype=np.int64)
    for h, ws in plan.items():
        walk = g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])]
        for w, (n, bases) in ws.items():
            a, b, c = (int(v) for v in walk[w:w + 3])
            row = [u for u in range(T.n_unique) if tuple(T.abc[u]) in ((a, b, c), (c, b, a))]
            assert len(row) == 1 and T.hap[row[0]] == h
            want[row[0]] = n * bases
    assert np.array_equal(tb, want)


def test_exact_restatement_on_known_values():
    e = hc.exact_stats([150] * 12 + [6000, 0], [300] * 14)
    assert e["nnz"] == 13 and e["mean"] == Fraction(26, 13) and max(e["z2"]) == 12 and len(e["kept"]) == 12 and e["mean_filtered"] == Fraction(1, 2)
    e = hc.exact_stats([150] * 9 + [6000], [300] * 10)
    assert max(e["z2"]) == 9 and len(e["kept"]) == 9          # ten values: the outlier sits at |z| = 3 exactly -- not a case any test may use
    e = hc.exact_stats([7, 7, 7], [300] * 3)
    assert e["var"] == 0 and e["z2"] is None and e["mean_filtered"] == 0
    assert hc.exact_stats([0, 0], [300, 300])["nnz"] == 0


def test_filter_cases_decide_what_they_claim():
    case, ref = hc.get_case("filters"), hc.get_case("filters").reference()
    mf, nnz = ref["mean_filtered"], ref["nnz"]
    assert nnz[:6].tolist() == [13, 9, 1, 13, 5, 13]
    assert mf[0] == 0.5                                        # the outlier went: the twelve 0.5 remain
    assert mf[1] == pytest.approx((8 * 0.5 + 20.0) / 9, rel=1e-15)   # nine values: kept
    assert mf[2] == 0.0 and mf[3] == 0.0 and mf[4] == 0.0 and mf[5] > 0.0
    z2 = hc.exact_stats(*case.hap_windows(0, 0))["z2"]
    assert max(z2) == 12 and hc.exact_stats(*case.hap_windows(0, 1))["z2"][-1] <= 8
    assert ref["has"][:6].tolist() == [3, 3, 1, 3, 3, 3] and ref["n_candidates"].tolist() == [5, 1]


def test_threshold_cases_decide_what_they_claim():
    ref = hc.get_case("thresholds").reference()
    assert ref["nnz"].tolist() == [3, 2, 10, 3] and ref["nt"].tolist() == [10] * 4 and ref["has"].tolist() == [3, 1, 3, 3]
    ref = hc.get_case("thresholds_shift").reference()
    assert ref["nnz"].tolist() == [3, 3, 8, 7, 2, 2, 1]
    assert ref["mean_filtered"][1] == 1.0 and ref["mean_filtered"][2] == 200.0 and ref["mean_filtered"][4] == 0.625 and ref["mean_filtered"][6] == 0.0
    assert 0.98 < ref["mean_filtered"][0] < 1.0
    assert ref["has"].tolist() == [3, 1, 3, 1, 3, 1, 3]
    assert hc.shift_threshold(0.3, 200.0, True) == 0.8 and hc.shift_threshold(0.3, 1.0, True) > 0.3 > hc.shift_threshold(0.3, float(ref["mean_filtered"][0]), True)


@pytest.mark.parametrize("name", [n for n in hc.CASE_NAMES if n.startswith("degenerate")])
def test_degenerate_cases_split_the_two_sum_shapes(name):
    """even haplotypes: only the sequential mean misses x (the oracle answers x); odd ones: only the pairwise tree misses it (the oracle answers 0.0)"""
    case = hc.get_case(name)
    ref = case.reference()
    counts = set()
    for h in range(case.species[0].n_paths):
        tb, ln = case.hap_windows(0, h)
        nz = tb[tb > 0]
        assert len(set(nz.tolist())) == 1 and 3 <= len(nz) <= 64
        x, c = float(nz[0]) / float(ln[0]), len(nz)
        seq, tree = hc.seq_sum(x, c) / c == x, hc.tree_sum(x, c) / c == x
        assert seq != tree and seq == (h % 2 == 1)
        assert (ref["mean_filtered"][h] == 0.0) == seq and ref["nnz"][h] == c
        counts.add(c)
    assert len(counts) >= 2


def test_chunk_and_queue_cases_lie_where_they_claim():
    """The layout the chunk cases aim at, derived from the oracle's table (rows walk after walk, as the path route files them) and the chunk rule: a change
    of either turns these assertions red instead of turning the cases into ordinary ones."""
    assert hc.chunk_rows(13, 299) == 128 and hc.chunk_rows(17, 391) == 192 and hc.chunk_rows(40, 920) == 320 and hc.chunk_rows(1025, 9225) == 8256
    assert hc.chunk_rows(10, 10 ** 7) == 1024 and hc.chunk_rows(1024, 9216) == 8192
    dense = hc.chunk_table(hc.get_case("chunks_dense"))
    assert [c[0] for c in dense] == [128, 128, 43] and [c[1] for c in dense] == [128, 128, 43]        # every row non-zero: pass 0's queue drains full batches of 64
    sparse = hc.chunk_table(hc.get_case("chunks_sparse"))
    assert [c[0] for c in sparse] == [128, 128, 43] and [c[1] for c in sparse] == [1, 0, 23]           # one non-zero row, none, the partial chunk full of them
    assert 12 in sparse[2][2] and 12 not in sparse[0][2] | sparse[1][2]                                  # haplotype 12 lies wholly in the last, partial chunk
    for name, rows in (("degenerate_17", [192, 192, 7]), ("degenerate_40", [320, 320, 280])):
        t = hc.chunk_table(hc.get_case(name))
        assert [c[0] for c in t] == rows
        across = (t[0][2] & t[1][2]) | (t[1][2] & t[2][2])                                                # haplotypes whose equal values are summed over two chunks
        assert across and all(hc.get_case(name).reference()["nnz"][h] >= 3 for h in across)
    for name, n in (("count_1024", 2), ("count_1025", 2), ("count_65", 2), ("count_64", 2)):
        assert len(hc.chunk_table(hc.get_case(name))) == n, name
    mixed = hc.get_case("mixed_1025_70_3")
    assert [len(hc.chunk_table(mixed, s)) for s in range(3)] == [2, 1, 1]
