"""tests/rescue_ref.py -- the yardstick of the GPU tests of the read rescue -- pinned on walks written and counted by hand: one walk of each of the six
outcomes, K = 0, J = 0, a contested read, a node visited twice, a read dropped by its flags, a species of 65."""
import numpy as np

from tests import rescue_ref as ref

# species 0: Sel = [h0, h1], Cand = [h2, h3, h4]; h5 is in neither list; node 10 is walked by h5 alone
H0 = [{0, 1, 2, 3, 9}, {2, 3, 4, 5}, {0, 1, 2, 3, 4, 5, 6}, {6, 7}, {7, 8}, {10}]
H1 = [{0, 1}]                      # K = 0, J = 1
H2 = [{0, 1}]                      # K = 1, J = 0
H3 = [{0} for _ in range(65)]      # K = 30, J = 35: skipped
HAP_NODES = [H0, H1, H2, H3]
SEL_OFF = [0, 2, 2, 3, 33]
SEL_HAP = [0, 1] + [] + [0] + list(range(30))
CAND_OFF = [0, 3, 4, 4, 39]
CAND_HAP = [2, 3, 4] + [0] + [] + list(range(30, 65))

READS = [
    (0, True, [0, 1, 2], 0, 10),       # compatible (h0)
    (0, True, [1, 4], 0, 10),          # mosaic, rescued by h2 alone
    (0, True, [9, 4], 0, 10),          # mosaic, no candidate walks node 9
    (0, True, [5, 6], 0, 10),          # foreign (node 6), rescued by h2 alone
    (0, True, [6, 8], 0, 10),          # foreign, patchwork: h2 / h3 walk 6, h4 walks 8
    (0, True, [0, 10], 0, 10),         # foreign, novel: nobody of either list walks 10
    (0, True, [7], 9, 3),              # foreign, rescued by h3 and h4: contested; pend < pstart: span 0
    (0, True, [6, 6, 5], 0, 10),       # node 6 twice: two foreign steps
    (0, False, [1, 4], 0, 10),         # dropped by its flags
    (-1, True, [], 0, 10),             # no species
    (1, True, [0, 1], 0, 5),           # K = 0: foreign, rescued
    (1, True, [0, 2], 0, 5),           # K = 0: foreign, novel
    (2, True, [0], 0, 5),              # J = 0: compatible
    (2, True, [0, 2], 0, 5),           # J = 0: foreign = foreign_novel
    (3, True, [0], 0, 5),              # 65: counted only
]


def _run():
    return ref.rescue(HAP_NODES, READS, SEL_OFF, SEL_HAP, CAND_OFF, CAND_HAP)


def test_six_outcomes_of_one_walk():
    s = lambda *x: set(x)
    assert ref.walk([s(0), s(0, 1)], [s(), s()]) == (ref.W_COMPATIBLE, set(), [0, 0, 0])
    assert ref.walk([s(1), s()], [s(0), s(0, 1)]) == (ref.W_FOREIGN_RESCUED, {0}, [1, 1, 0])
    assert ref.walk([s(), s()], [s(0, 1), s(2)]) == (ref.W_FOREIGN_PATCHWORK, set(), [2, 2, 0])
    assert ref.walk([s(0), s()], [s(0), s()]) == (ref.W_FOREIGN_NOVEL, set(), [1, 0, 1])
    assert ref.walk([s(0), s(1)], [s(0), s(0)]) == (ref.W_MOSAIC_RESCUED, {0}, [0, 0, 0])
    assert ref.walk([s(0), s(1)], [s(), s(0)]) == (ref.W_MOSAIC_UNRESCUED, set(), [0, 0, 0])
    # a compatible walk may be walked by a candidate too: it is not unexplained, so it is not rescued
    assert ref.walk([s(0)], [s(3)]) == (ref.W_COMPATIBLE, {3}, [0, 0, 0])


def test_species_counts_by_hand():
    species, step, cand, cand_steps = _run()
    assert species.shape == (4, 9, 3) and step.shape == (4, 3) and cand.shape == (39, 3, 3) and cand_steps.shape == (39,)
    assert species[0].tolist() == [[8, 17, 70], [1, 3, 10], [5, 10, 40], [3, 6, 20], [1, 2, 10], [1, 2, 10], [2, 4, 20], [1, 2, 10], [1, 1, 0]]
    assert step[0].tolist() == [7, 6, 1]
    assert cand[0].tolist() == [[3, 7, 30], [3, 7, 30], [2, 5, 20]]          # h2: rescued, alone, from_foreign
    assert cand[1].tolist() == [[1, 1, 0], [0, 0, 0], [1, 1, 0]]             # h3: the contested read only
    assert cand[2].tolist() == [[1, 1, 0], [0, 0, 0], [1, 1, 0]]
    assert cand_steps[:3].tolist() == [4, 5, 2]


def test_k0_j0_and_a_species_of_65():
    species, step, cand, cand_steps = _run()
    # K = 0: every counted read is foreign
    assert species[1].tolist() == [[2, 4, 10], [0, 0, 0], [2, 4, 10], [1, 2, 5], [0, 0, 0], [1, 2, 5], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert step[1].tolist() == [4, 3, 1] and cand[3].tolist() == [[1, 2, 5], [1, 2, 5], [1, 2, 5]] and cand_steps[3] == 3
    # J = 0: foreign = foreign_novel, no rescue
    assert species[2].tolist() == [[2, 3, 10], [1, 1, 5], [1, 2, 5], [0, 0, 0], [0, 0, 0], [1, 2, 5], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert step[2].tolist() == [1, 0, 1]
    # K + J = 65: counted only
    assert species[3].tolist() == [[1, 1, 5]] + [[0, 0, 0]] * 8 and not step[3].any() and not cand[4:].any() and not cand_steps[4:].any()


def test_identities_hold_and_catch():
    species, step, cand, cand_steps = _run()
    ref.check_identities(species, step, cand, cand_steps, SEL_OFF, CAND_OFF)
    broken = species.copy()
    broken[0, ref.MOSAIC, 0] += 1
    try:
        ref.check_identities(broken, step, cand, cand_steps, SEL_OFF, CAND_OFF)
    except AssertionError:
        pass
    else:
        raise AssertionError("check_identities passes a broken count")


def test_rank():
    species, step, cand, cand_steps = _run()
    assert ref.rank(CAND_HAP[:3], cand[:3]) == [0, 1, 2]                     # span 30 first; the tie of h3 and h4 by haplotype index
    assert ref.rank([2, 9, 4], cand[:3]) == [0, 2, 1]
    assert ref.rank(CAND_HAP[:3], cand[:3], top=2) == [0, 1]
    none = np.zeros((2, 3, 3), dtype=np.uint64)
    assert ref.rank([0, 1], none) == []                                      # a candidate that rescues no read is left out
