"""Pins tests/pair_evidence_ref.py, the numpy restatement of pantax_hip_strain_pair_evidence the GPU tests compare against, on a case worked by hand, and
its identities against the references of the two calls it joins (tests/evidence_ref.py, tests/hap_pairs_ref.py) on seeded random species.  No GPU."""
import types

import numpy as np

from tests.evidence_ref import species_evidence
from tests.hap_pairs_ref import derived, species_pairs
from tests.pair_evidence_ref import HEADER, MAX_K, only, pair_class, pair_evidence, species_pair_evidence, table

# six nodes, four haplotypes: h1 is h0 backwards with a node repeated (identical), h2 a part of h0 and of h3 (nested), h3 shares node 0 with h0 (distinct);
# node 1 has no length, node 5 is walked by nobody
NODE_LEN = [5, 0, 7, 3, 11, 2]
COV = [5, 0, 4, 0, 11, 1]
BASES = [50, 0, 9, 0, 33, 1]
WALKS = [[0, 1, 2], [2, 1, 0, 0], [0], [3, 4, 0]]


def test_hand_case():
    pair, sp = species_pair_evidence(NODE_LEN, WALKS, COV, BASES)
    assert pair.dtype == sp.dtype == np.uint64 and pair.shape == (4, 4, 4) and sp.shape == (3, 4)
    h0, n0, h3 = [3, 12, 9, 59], [1, 5, 5, 50], [3, 19, 16, 83]              # nodes {0, 1, 2}; node 0 alone; nodes {0, 3, 4}
    exp = [[h0, h0, n0, n0],
           [h0, h0, n0, n0],
           [n0, n0, n0, n0],
           [n0, n0, n0, h3]]
    assert pair.tolist() == exp
    assert sp.tolist() == [[6, 28, 21, 93], [1, 2, 1, 1], [1, 5, 5, 50]]     # total; orphan = node 5; core = node 0
    assert only(pair, 0, 3).tolist() == [2, 7, 4, 9] and only(pair, 3, 0).tolist() == [2, 14, 11, 33]
    assert only(pair, 0, 2).tolist() == [2, 7, 4, 9] and only(pair, 2, 0).tolist() == [0, 0, 0, 0]
    assert not only(pair, 0, 1).any() and not only(pair, 1, 0).any()
    assert [pair_class(pair, a, b) for a, b in ((0, 1), (0, 2), (2, 3), (0, 3), (1, 3))] == ["identical", "nested", "nested", "distinct", "distinct"]
    # the class looks at the len column alone: a haplotype that lacks only the node without length is identical to h0
    p2, _ = species_pair_evidence(NODE_LEN, [WALKS[0], [0, 2]], COV, BASES)
    assert only(p2, 0, 1).tolist() == [1, 0, 0, 0] and pair_class(p2, 0, 1) == "identical"
    # nothing selected; one selected
    p0, s0 = species_pair_evidence(NODE_LEN, [], COV, BASES)
    assert p0.shape == (0, 0, 4) and s0.tolist() == [[6, 28, 21, 93], [6, 28, 21, 93], [0, 0, 0, 0]]
    p1, s1 = species_pair_evidence(NODE_LEN, [WALKS[3]], COV, BASES)
    assert p1.tolist() == [[h3]] and s1[2].tolist() == h3


def test_hand_case_wraps_as_u64():
    big = [2 ** 63, 0, 2 ** 63 + 5, 0, 0, 0]
    pair, sp = species_pair_evidence(NODE_LEN, WALKS[:1], COV, big)
    assert int(pair[0, 0, 3]) == 5 and int(sp[0, 3]) == 5


def test_hand_case_table():
    pair, _ = species_pair_evidence(NODE_LEN, WALKS, COV, BASES)
    entries = [("t%d" % h, "g%d" % h, np.float64(w)) for h, w in enumerate((8.0, 0.5, 3.25, 2.0))]
    many = [("t", "g", np.float64(1.0))] * (MAX_K + 1)
    rows = table([("9", entries[:1], pair[:1, :1]), ("10", entries, pair), ("11", many, None), ("12", [], None)])
    assert rows[0] == HEADER and all(len(r) == len(HEADER) == 14 for r in rows)
    assert len(rows) == 1 + 3 * 6 + 1
    assert rows[-1] == ["11", "-", "-", "-", "-", "skipped"] + ["-"] * 8
    assert [(r[1], r[3], r[5]) for r in rows[1:4]] == [("t0", "t1", "shared"), ("t0", "t1", "only"), ("t1", "t0", "only")]
    assert [r[13] for r in rows[1:4]] == ["identical"] * 3 and rows[1][12] == 8.5 and rows[2][12] == 8.0 and rows[3][12] == 0.5
    assert rows[1][6:12] == ["3", "12", "9", "59", np.float64(59) / np.float64(12), np.float64(9) / np.float64(12)]
    assert rows[2][6:12] == ["0", "0", "0", "0", "-", "-"]                   # nothing only h0 walks against its twin: no length, no ratio
    pairs = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    at = 1 + 3 * pairs.index((0, 3))
    assert rows[at][:6] == ["10", "t0", "g0", "t3", "g3", "shared"] and rows[at][6:10] == ["1", "5", "5", "50"] and rows[at][12] == 10.0
    assert rows[at + 1][:6] == ["10", "t0", "g0", "t3", "g3", "only"] and rows[at + 1][6:10] == ["2", "7", "4", "9"] and rows[at + 1][12] == 8.0
    assert rows[at + 2][:6] == ["10", "t3", "g3", "t0", "g0", "only"] and rows[at + 2][6:10] == ["2", "14", "11", "33"] and rows[at + 2][12] == 2.0
    assert {r[13] for r in rows[at:at + 3]} == {"distinct"}


def test_identities_on_random_species():
    rng = np.random.default_rng(20261019)
    for V, H, K in ((200, 5, 5), (777, 9, 4), (64, 3, 1), (300, 70, 70)):
        node_len = rng.integers(0, 50, V)
        cov = (node_len * rng.random(V)).astype(np.int64)                    # covered <= len
        bases = rng.integers(0, 2 ** 40, V)
        walks = [rng.integers(0, V, rng.integers(1, 2 * V)) for _ in range(H)]
        sel = [walks[int(h)] for h in rng.permutation(H)[:K]]
        pair, sp = species_pair_evidence(node_len, sel, cov, bases)
        hp, hsp = species_pairs(node_len, sel)
        ev, esp = species_evidence(node_len, sel, cov, bases)
        assert np.array_equal(pair[:, :, :2], hp)                            # columns 0:2 = the db-only call
        assert np.array_equal(np.einsum("iiq->iq", pair), ev[:, 0])          # the diagonal = the evidence call's all
        assert np.array_equal(sp, esp) and np.array_equal(sp[:, :2], hsp)
        d = np.einsum("iiq->iq", pair)
        assert np.array_equal(pair, pair.transpose(1, 0, 2))
        assert np.all(pair <= np.minimum(d[:, None], d[None, :])) and np.all(sp[2] <= pair)
        for a in range(K):
            for b in range(a + 1, K):
                assert pair_class(pair, a, b) == derived(hp, a, b)[3]
        if K >= 2:                                                           # private = what a walks and no other: never more than only_a against any b
            assert all(np.all(ev[a, 1] <= only(pair, a, b)) for a in range(K) for b in range(K) if a != b)
    g = types.SimpleNamespace(node_len=np.array(NODE_LEN), path_off=np.array([0, 3, 7, 8, 11]), path_nodes=np.concatenate(WALKS))
    off, pair, sp = pair_evidence([g, g], [0, 2, 2], [3, 0], np.array(COV * 2), np.array(BASES + [0] * 6))
    assert off.tolist() == [0, 4, 4] and pair.shape == (4, 4) and pair[1].tolist() == [1, 5, 5, 50] and sp.shape == (2, 3, 4) and int(sp[1, 0, 3]) == 0
