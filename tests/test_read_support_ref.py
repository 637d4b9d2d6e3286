"""The row-by-row reading of the per-strain read support contract (tests/read_support_ref.py) on cases worked out by hand, and the identities of the
contract on random small inputs.  No GPU."""
import numpy as np

from tests.read_support_ref import check_identities, read_support


def test_hand_case():
    # species 0: five nodes, h0 = {0,1,2}, h1 = {0,1,3}, h2 = {0,4}; candidates in the order h2, h0, h1 with weights 1, 2, 2 (h0 and h1 tie)
    # species 1: no candidates; species 2: one candidate
    hap_nodes = [[{0, 1, 2}, {0, 1, 3}, {0, 4}], [{0}], [{0, 1}]]
    cand_off, cand_hap, cand_w = [0, 3, 3, 4], [2, 0, 1, 0], [1.0, 2.0, 2.0, 3.0]
    reads = [
        (0, True, [0], 10, 25),        # every candidate: ambiguous and uninformative; assigned to h0 (tie with h1: the smaller index)
        (0, True, [1, 0, 1], 0, 30),   # a node twice: N = {0, 1}: h0 and h1; assigned to h0
        (0, True, [2], 5, 5),          # h0 alone
        (0, True, [4, 0], 7, 3),       # h2 alone; pend < pstart: span 0
        (0, True, [3, 4], 0, 100),     # no candidate
        (0, False, [0], 0, 50),        # dropped: not counted
        (-1, True, [0], 0, 50),        # "U"
        (1, True, [0], 0, 9),          # a species without candidates: counted only
        (2, True, [0, 1], 2, 12),
        (2, True, [2], 0, 4),
    ]
    hap, species, pair_off, pair = read_support(hap_nodes, reads, cand_off, cand_hap, cand_w)
    assert hap.dtype == species.dtype == pair_off.dtype == pair.dtype == np.uint64
    assert hap.tolist() == [
        [[2, 3, 15], [1, 2, 0], [1, 2, 0]],      # h2: compatible, unique, assigned
        [[3, 5, 45], [1, 1, 0], [3, 5, 45]],     # h0
        [[2, 4, 45], [0, 0, 0], [0, 0, 0]],      # h1
        [[1, 2, 10], [1, 2, 10], [1, 2, 10]],    # species 2, h0
    ]
    assert species.tolist() == [
        [[5, 9, 145], [1, 2, 100], [2, 4, 45], [1, 1, 15]],   # counted, unexplained, ambiguous, uninformative
        [[1, 1, 9], [0, 0, 0], [0, 0, 0], [0, 0, 0]],
        [[2, 3, 14], [1, 1, 4], [0, 0, 0], [1, 2, 10]],
    ]
    assert pair_off.tolist() == [0, 9, 9, 10]
    assert pair.tolist() == [2, 1, 1, 1, 3, 2, 1, 2, 2, 1]
    check_identities(hap, species, pair_off, pair, cand_off)


def test_wide_species_owns_no_pair_block():
    # 66 candidates: no pair block; a read of node 0 is compatible with the 33 even haplotypes, assigned to the heaviest (haplotype 64)
    hap_nodes = [[{0} if h % 2 == 0 else {1} for h in range(70)], [{0}, {0}]]
    cand_hap = list(range(65, -1, -1)) + [1, 0]
    cand_w = [float(h) for h in cand_hap[:66]] + [1.0, 1.0]
    cand_off = [0, 66, 68]
    reads = [(0, True, [0], 0, 7), (0, True, [0, 1], 0, 1), (1, True, [0], 3, 8)]
    hap, species, pair_off, pair = read_support(hap_nodes, reads, cand_off, cand_hap, cand_w)
    assert pair_off.tolist() == [0, 0, 4] and pair.tolist() == [1, 1, 1, 1]
    assert hap[:66, 0, 0].tolist() == [1 if h % 2 == 0 else 0 for h in cand_hap[:66]]
    assert hap[:66, 2, 0].tolist() == [1 if h == 64 else 0 for h in cand_hap[:66]] and hap[:66, 1].sum() == 0
    assert species[0].tolist() == [[2, 3, 8], [1, 2, 1], [1, 1, 7], [0, 0, 0]]
    assert hap[66:].tolist() == [[[1, 1, 5], [0, 0, 0], [0, 0, 0]], [[1, 1, 5], [0, 0, 0], [1, 1, 5]]]   # equal weights: haplotype 0, the second entry
    assert species[1].tolist() == [[1, 1, 5], [0, 0, 0], [1, 1, 5], [1, 1, 5]]
    check_identities(hap, species, pair_off, pair, cand_off)


def test_identities_on_random_inputs():
    rng = np.random.default_rng(7)
    for _ in range(40):
        S = int(rng.integers(1, 5))
        hap_nodes, cand_off, cand_hap, cand_w = [], [0], [], []
        for s in range(S):
            V, H = int(rng.integers(2, 9)), int(rng.integers(1, 6))
            hap_nodes.append([set(rng.choice(V, size=int(rng.integers(1, V + 1)), replace=False).tolist()) for _ in range(H)])
            ks = rng.permutation(H)[: int(rng.integers(0, H + 1))].tolist()
            cand_hap += ks
            cand_w += rng.choice([0.5, 1.0, 2.0], size=len(ks)).tolist()
            cand_off.append(len(cand_hap))
        reads = []
        for _ in range(60):
            s = int(rng.integers(-1, S))
            V = max(len(set().union(*hap_nodes[s])), 2) if s >= 0 else 2
            reads.append((s, bool(rng.random() < 0.9), rng.integers(0, V, size=int(rng.integers(1, 5))).tolist(), int(rng.integers(0, 50)), int(rng.integers(0, 200))))
        out = read_support(hap_nodes, reads, cand_off, cand_hap, cand_w)
        check_identities(*out, cand_off)
        assert int(out[1][:, 0, 0].sum()) == sum(1 for r in reads if r[0] >= 0 and r[1])
