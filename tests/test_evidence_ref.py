"""Pins the numpy restatement of the node-evidence contract (tests/evidence_ref.py) on a micro case computed by hand, so that the GPU tests,
which compare the library with it, cannot agree with a wrong reading of the contract."""
import numpy as np

from tests.evidence_ref import evidence, species_evidence

# eight nodes, three haplotypes: node 6 is walked by nobody, node 1 twice by haplotype 0, nodes 0 and 7 by all three;
# node 2 by haplotypes 0 and 2, nodes 3 and 4 only by haplotype 1, node 5 only by haplotype 2
NODE_LEN = np.array([5, 3, 7, 2, 4, 6, 1, 8])
COV = np.array([5, 0, 7, 1, 4, 3, 0, 2])
BASES = np.array([50, 0, 21, 1, 40, 9, 0, 2])
WALKS = [[0, 1, 2, 1, 7], [0, 3, 4, 7], [0, 2, 5, 7]]
TOTAL = [8, 36, 22, 123]


def _run(sel):
    hap, sp = species_evidence(NODE_LEN, [WALKS[h] for h in sel], COV, BASES)
    assert hap.dtype == sp.dtype == np.uint64 and hap.shape == (len(sel), 2, 4) and sp.shape == (3, 4)
    # the identities of the contract, whatever the selection
    assert sp[0].tolist() == TOTAL
    assert np.all(hap[:, 1] <= hap[:, 0])                                     # private <= all, component-wise
    assert np.all(hap[:, 1].sum(axis=0) + sp[1] <= sp[0])                     # private sets and the orphans are disjoint
    return hap.tolist(), sp.tolist()


def test_micro_empty_selection():
    hap, sp = _run([])
    assert hap == [] and sp == [TOTAL, TOTAL, [0, 0, 0, 0]]                   # everything is orphan, no core without a selection


def test_micro_one_selected():
    hap, sp = _run([1])                                                       # nodes 0 3 4 7
    assert hap == [[[4, 19, 12, 93], [4, 19, 12, 93]]]                        # K = 1: all = private ...
    assert sp == [TOTAL, [4, 17, 10, 30], [4, 19, 12, 93]]                    # ... = core; orphan = nodes 1 2 5 6
    assert (np.array(sp[1]) + np.array(hap[0][0])).tolist() == TOTAL          # total = orphan + the nodes with m >= 1


def test_micro_two_of_three_in_given_order():
    hap, sp = _run([2, 0])
    assert hap == [[[4, 26, 17, 82], [1, 6, 3, 9]],                           # haplotype 2: nodes 0 2 5 7; private: node 5
                   [[4, 23, 14, 73], [1, 3, 0, 0]]]                           # haplotype 0: nodes 0 1 2 7 (node 1 once); private: node 1
    assert sp == [TOTAL, [3, 7, 5, 41], [3, 20, 14, 73]]                      # orphan: nodes 3 4 6; core: nodes 0 2 7
    covered = [5, 29, 17, 82]                                                 # nodes 0 1 2 5 7: m >= 1
    assert (np.array(sp[1]) + np.array(covered)).tolist() == TOTAL


def test_micro_all_selected():
    hap, sp = _run([0, 1, 2])
    assert hap == [[[4, 23, 14, 73], [1, 3, 0, 0]], [[4, 19, 12, 93], [2, 6, 5, 41]], [[4, 26, 17, 82], [1, 6, 3, 9]]]
    assert sp == [TOTAL, [1, 1, 0, 0], [2, 13, 7, 52]]                        # orphan: node 6; core: nodes 0 7
    covered = [7, 35, 22, 123]
    assert (np.array(sp[1]) + np.array(covered)).tolist() == TOTAL


def test_micro_species_offsets_and_order():
    class G:
        def __init__(self, node_len, walks):
            self.node_len = np.array(node_len)
            self.path_off = np.concatenate([[0], np.cumsum([len(w) for w in walks])]).astype(np.uint64)
            self.path_nodes = np.array([v for w in walks for v in w], dtype=np.uint32)
    species = [G([3, 4], [[0, 1], [1]]), G(NODE_LEN, WALKS), G([9], [[0]])]
    cov = np.concatenate([[1, 2], COV, [4]])
    bases = np.concatenate([[5, 6], BASES, [7]])
    # species 0: haplotype 1; species 1: haplotypes 2 then 0; species 2: nothing
    hap, sp = evidence(species, [0, 1, 3, 3], [1, 2, 0], cov, bases)
    assert hap.tolist() == [[[1, 4, 2, 6], [1, 4, 2, 6]], [[4, 26, 17, 82], [1, 6, 3, 9]], [[4, 23, 14, 73], [1, 3, 0, 0]]]
    assert sp.tolist() == [[[2, 7, 3, 11], [1, 3, 1, 5], [1, 4, 2, 6]], [TOTAL, [3, 7, 5, 41], [3, 20, 14, 73]], [[1, 9, 4, 7], [1, 9, 4, 7], [0, 0, 0, 0]]]
