"""Pins the numpy restatement of the near-miss contract (tests/near_miss_ref.py) on a micro case computed by hand and on the contract's identities, and the
host helper pantax_hip_near_miss_rank (through ctypes: it needs no GPU) on hand-written orders -- so that the GPU tests, which compare the library with
near_miss_ref, cannot agree with a wrong reading of the contract."""
import ctypes as C

import numpy as np
import pytest

from tests.evidence_ref import species_evidence
from tests.near_miss_ref import near_miss, near_miss_rank, species_near_miss

E_INVALID = -1

# eight nodes, four haplotypes: node 6 is walked by nobody, node 1 twice by haplotype 0, node 4 twice by haplotype 3, node 3 has no length.
#   node      0        1    2      3      4      5      6   7
#   walked by 0 1 2 3  0    0 2    1 3    1 3    2 3    -   0 1 2
NODE_LEN = np.array([5, 3, 7, 0, 4, 6, 1, 8])
COV = np.array([5, 0, 7, 0, 4, 3, 0, 2])
BASES = np.array([50, 0, 21, 0, 40, 9, 0, 2])
WALKS = [[0, 1, 2, 1, 7], [0, 3, 4, 7], [0, 2, 5, 7], [0, 4, 4, 5, 3]]
Z = [0, 0, 0, 0]


def _run(sel, cand):
    c, sp = species_near_miss(NODE_LEN, [WALKS[h] for h in sel], [WALKS[h] for h in cand], COV, BASES)
    assert c.dtype == sp.dtype == np.uint64 and c.shape == (len(cand), 2, 4) and sp.shape == (3, 4)
    return c.tolist(), sp.tolist()


def test_micro_one_reported_three_candidates_in_given_order():
    cand, sp = _run([0], [3, 1, 2])                                          # orphans: nodes 3 4 5 6; every claimed one has two candidates
    assert sp == [[4, 11, 7, 49], [3, 10, 7, 49], [3, 10, 7, 49]]            # node 6 is an orphan nobody claims
    assert cand == [[[3, 10, 7, 49], Z], [[2, 4, 4, 40], Z], [[1, 6, 3, 9], Z]]   # haplotype 3: nodes 3 4 5 (node 4 once); 1: nodes 3 4; 2: node 5


def test_micro_exclusive_beside_contested():
    cand, sp = _run([0], [3, 1])                                             # node 5 is now haplotype 3's alone
    assert sp == [[4, 11, 7, 49], [3, 10, 7, 49], [2, 4, 4, 40]]
    assert cand == [[[3, 10, 7, 49], [1, 6, 3, 9]], [[2, 4, 4, 40], Z]]


def test_micro_disjoint_candidates():
    cand, sp = _run([2], [1, 0])                                             # orphans: nodes 1 3 4 6; node 1 is haplotype 0's (walked twice: once), 3 4 haplotype 1's
    assert sp == [[4, 8, 4, 40], [3, 7, 4, 40], Z]
    assert cand == [[[2, 4, 4, 40], [2, 4, 4, 40]], [[1, 3, 0, 0], [1, 3, 0, 0]]]


def test_micro_nothing_reported():
    cand, sp = _run([], [0, 1, 2, 3])                                        # every node is an orphan; only node 1 has a single candidate
    assert sp == [[8, 34, 21, 122], [7, 33, 21, 122], [6, 30, 21, 122]]
    assert cand == [[[4, 23, 14, 73], [1, 3, 0, 0]], [[4, 17, 11, 92], Z], [[4, 26, 17, 82], Z], [[4, 15, 12, 99], Z]]


def test_micro_single_candidate_and_empty_sets():
    cand, sp = _run([0], [1])                                                # J = 1: novel = exclusive = claimed, nothing contested
    assert sp == [[4, 11, 7, 49], [2, 4, 4, 40], Z] and cand == [[[2, 4, 4, 40], [2, 4, 4, 40]]]
    cand, sp = _run([0], [])
    assert cand == [] and sp == [[4, 11, 7, 49], Z, Z]
    cand, sp = _run([], [])
    assert cand == [] and sp == [[8, 34, 21, 122], Z, Z]
    cand, sp = _run([0, 3], [2, 1])                                          # only node 6 is left, and nobody walks it
    assert sp == [[1, 1, 0, 0], Z, Z] and cand == [[Z, Z], [Z, Z]]


def _random_species(rng, V, H):
    node_len = rng.integers(0, 50, V)
    cov = np.minimum(node_len, rng.integers(0, 50, V))
    bases = cov * rng.integers(0, 30, V)
    walks = [rng.integers(0, V, int(rng.integers(1, 2 * V))) for _ in range(H)]   # repeats and unvisited nodes both happen
    return node_len, cov, bases, walks


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_identities_on_random_species(seed):
    rng = np.random.default_rng(seed)
    node_len, cov, bases, walks = _random_species(rng, 40, 9)
    order = rng.permutation(9)
    K = int(rng.integers(0, 5))
    sel, cnd = [int(h) for h in order[:K]], [int(h) for h in order[K:K + int(rng.integers(1, 9 - K + 1))]]
    cand, sp = species_near_miss(node_len, [walks[h] for h in sel], [walks[h] for h in cnd], cov, bases)
    orphan, claimed, contested = sp
    assert np.all(cand[:, 1] <= cand[:, 0])                                                  # exclusive <= novel
    assert np.array_equal(claimed, contested + cand[:, 1].sum(axis=0, dtype=np.uint64))      # claimed = contested + the exclusive sums
    assert np.all(contested <= claimed) and np.all(claimed <= orphan)
    ev_sel = species_evidence(node_len, [walks[h] for h in sel], cov, bases)[1]
    assert np.array_equal(orphan, ev_sel[1])                                                 # the evidence call's orphan of the same Sel
    ev_cand = species_evidence(node_len, [walks[h] for h in cnd], cov, bases)[0]
    assert np.all(cand[:, 0] <= ev_cand[:, 0])                                               # novel <= all of the same haplotype
    one, sp1 = species_near_miss(node_len, [walks[h] for h in sel], [walks[cnd[0]]], cov, bases)   # J = 1
    assert np.array_equal(one[0, 0], one[0, 1]) and np.array_equal(one[0, 0], sp1[1]) and not sp1[2].any()
    assert np.array_equal(one[0, 0], cand[0, 0])                                             # novel does not depend on the other candidates
    none, sp0 = species_near_miss(node_len, [], [walks[h] for h in cnd], cov, bases)         # Sel empty: every node is an orphan
    assert sp0[0].tolist() == [40, int(node_len.sum()), int(cov.sum()), int(bases.sum())]


def test_species_offsets_and_order():
    class G:
        def __init__(self, node_len, walks):
            self.node_len = np.array(node_len)
            self.path_off = np.concatenate([[0], np.cumsum([len(w) for w in walks])]).astype(np.uint64)
            self.path_nodes = np.array([v for w in walks for v in w], dtype=np.uint32)
    species = [G([3, 4], [[0, 1], [1]]), G(NODE_LEN, WALKS), G([9], [[0]])]
    cov = np.concatenate([[1, 2], COV, [4]])
    bases = np.concatenate([[5, 6], BASES, [7]])
    # species 0: haplotype 1 reported, 0 a candidate; species 1: 0 reported, 3 then 1 candidates; species 2: its one haplotype a candidate
    cand, sp = near_miss(species, [0, 1, 2, 2], [1, 0], [0, 1, 3, 4], [0, 3, 1, 0], cov, bases)
    assert cand.tolist() == [[[1, 3, 1, 5], [1, 3, 1, 5]], [[3, 10, 7, 49], [1, 6, 3, 9]], [[2, 4, 4, 40], Z], [[1, 9, 4, 7], [1, 9, 4, 7]]]
    assert sp.tolist() == [[[1, 3, 1, 5], [1, 3, 1, 5], Z], [[4, 11, 7, 49], [3, 10, 7, 49], [2, 4, 4, 40]], [[1, 9, 4, 7], [1, 9, 4, 7], Z]]


# ---- pantax_hip_near_miss_rank ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from pantax_amd import _ffi
    return _ffi.load()


def _c_rank(lib, haps, novel, top, preset=99):
    """novel: per candidate (covered, bases) -> (rc, order, n); rank_out and n_out are pre-filled with `preset`"""
    ch = np.ascontiguousarray(haps, dtype=np.uint32)
    co = np.zeros((len(haps), 2, 4), dtype=np.uint64)
    for c, (cv, bs) in enumerate(novel):
        co[c, 0] = [1, 10, cv, bs]
        co[c, 1] = [7, 7, 7, 7 + c]                                          # exclusive takes no part in the order
    out = np.full(max(len(haps), 1), preset, dtype=np.uint32)
    n = C.c_uint32(preset)
    rc = lib.pantax_hip_near_miss_rank(len(haps), ch.ctypes.data_as(C.c_void_p), co.ctypes.data_as(C.c_void_p), top, out.ctypes.data_as(C.c_void_p), C.byref(n))
    return rc, out, int(n.value), ch, co


# haplotype indices in no order; (covered, bases) of novel
HAPS = [9, 4, 7, 2, 5, 11]
NOVEL = [(3, 50), (8, 50), (8, 50), (1, 0), (2, 90), (8, 50)]
# bases 90 first (position 4); then the four with 50: covered 8 before covered 3, the three with covered 8 by haplotype index 4 < 7 < 11 = positions
# 1, 2, 5; then position 0; position 3 has no novel bases and is left out
ORDER = [4, 1, 2, 5, 0]


def test_rank_order_ties_and_zero_bases(lib):
    rc, out, n, ch, co = _c_rank(lib, HAPS, NOVEL, 0)
    assert rc == 0 and n == 5 and out[:5].tolist() == ORDER and out[5] == 99
    assert near_miss_rank(ch, co, 0) == ORDER                                # the restatement the GPU tests use
    from pantax_amd.engine import near_miss_rank as engine_rank
    assert engine_rank(ch, co).tolist() == ORDER and engine_rank(ch, co, top=2).tolist() == ORDER[:2]


@pytest.mark.parametrize("top,expect", [(0, ORDER), (1, ORDER[:1]), (3, ORDER[:3]), (5, ORDER), (6, ORDER), (100, ORDER)])
def test_rank_top(lib, top, expect):
    rc, out, n, ch, co = _c_rank(lib, HAPS, NOVEL, top)
    assert rc == 0 and n == len(expect) and out[:n].tolist() == expect and np.all(out[n:] == 99)
    assert near_miss_rank(ch, co, top) == expect


def test_rank_nothing_to_rank(lib):
    rc, out, n, _, _ = _c_rank(lib, [3, 1], [(5, 0), (9, 0)], 0)             # covered without bases does not count
    assert rc == 0 and n == 0 and np.all(out == 99)
    rc, out, n, _, _ = _c_rank(lib, [], [], 4)
    assert rc == 0 and n == 0


def test_rank_null_pointers(lib):
    ch = np.array(HAPS, dtype=np.uint32)
    co = np.ones((6, 2, 4), dtype=np.uint64)
    out = np.full(6, 99, dtype=np.uint32)
    n = C.c_uint32(99)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for args in ((None, vp(co), 0, vp(out), C.byref(n)), (vp(ch), None, 0, vp(out), C.byref(n)), (vp(ch), vp(co), 0, None, C.byref(n)), (vp(ch), vp(co), 0, vp(out), None)):
        assert lib.pantax_hip_near_miss_rank(6, *args) == E_INVALID
    assert np.all(out == 99) and n.value == 99
