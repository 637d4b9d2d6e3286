"""tests/links_ref.py, the yardstick of the link support tests, pinned on cases small enough to do by hand.  No GPU."""
import numpy as np

from tests import links_ref as ref

u64 = lambda x: np.array(x, dtype=np.uint64)

# one species of six nodes, lengths 10 .. 60; three haplotypes:
#   h0 = 0 1 2 3      h1 = 0 1 3 1      h2 = 4
WALKS = [[[0, 1, 2, 3], [0, 1, 3, 1], [4]]]
NODE_LEN = [[10, 20, 30, 40, 50, 60]]
BASES = [[100, 40, 0, 120, 50, 7]]                                        # depth 10, 2, 0, 3, 1, 0


def rd(nodes, counted=True, sp=0):
    return (sp, counted, nodes, 0, 10)


def test_crossing_classes_by_hand():
    assert ref.crossing_class(True, set(), set()) == ref.KNOWN
    assert ref.crossing_class(False, {0}, {0, 1}) == ref.SKIP
    assert ref.crossing_class(False, {0}, {1}) == ref.SWITCH
    assert ref.crossing_class(False, set(), {1}) == ref.FOREIGN and ref.crossing_class(False, {1}, set()) == ref.FOREIGN
    assert ref.crossings([1, 1, 2, 0, 3, 3], [1, 0, 0, 0, 0], 2) == [1, 1, 1, 2]
    assert ref.crossings([1 << 63, 1 << 63], [0], 64) == [0, 1, 0, 0] and ref.crossings([1 << 63, 1 << 63], [0], 63) == [0, 0, 0, 1]
    assert ref.crossings([5], [], 3) == [0, 0, 0, 0] and ref.crossings([7, 7], [0], 0) == [0, 0, 0, 1]
    assert ref.link(3, 1) == ref.link(1, 3) == (1, 3) and ref.link(2, 2) == (2, 2)


def test_top_order_by_hand():
    assert ref.top([5, 9, 5, 9, 1], [40, 30, 10, 20, 0]) == [3, 1, 2, 0, 4]
    assert ref.top([5, 9, 5, 9, 1], [40, 30, 10, 20, 0], 2) == [3, 1]
    assert ref.top([7, 7, 7], [3, 3, 1]) == [2, 0, 1] and ref.top([], []) == []


def test_two_strains_by_hand():
    """Sel = [h1, h0]: position 0 is h1, position 1 is h0.  Links: {0,1} by both (core), {1,2} and {2,3} by h0 alone, {1,3} by h1 alone -- at two
    positions of its walk."""
    reads = [rd([0, 1]), rd([1, 0]),                                       # {0,1} twice, once in reverse
             rd([3, 1, 3]),                                                # {1,3} twice
             rd([0, 3]),                                                   # both strains walk 0 and 3, never adjacent: skip
             rd([2, 4]),                                                   # nobody of the list walks 4: foreign
             rd([5]),                                                      # a single step: counted, no crossing
             rd([0, 1], counted=False), rd([0, 1], sp=-1)]                 # dropped / unbinned
    species, table, hap, brk_off, rec = ref.links(WALKS, NODE_LEN, BASES, reads, u64([0, 2]), np.array([1, 0], dtype=np.uint32))
    assert species.tolist() == [[6, 6, 4, 1, 0, 1]]
    assert table.tolist() == [[4, 2, 1, 1]]
    # h1 = 0 1 3 1: {0,1} crossed (2), {1,3} crossed (2), {3,1} crossed (2); {1,3} is private to position 0
    # h0 = 0 1 2 3: {0,1} crossed (2), {1,2}: bases[2] = 0 -> open, {2,3}: open; both private to position 1
    assert hap.tolist() == [[3, 3, 0, 0, 2, 2, 0, 6], [3, 1, 2, 0, 2, 0, 0, 2]]
    assert brk_off.tolist() == [0, 0, 0] and rec == []
    ref.check_identities(species, table, hap, brk_off, [4, 4], u64([0, 2]))


def test_breaks_switch_and_single_strain_by_hand():
    """Sel = [h0, h2]: h0's links {0,1}, {1,2}, {2,3}; h2 has one step and no link.  bases[2] > 0 here."""
    bases = [[100, 40, 90, 120, 50, 7]]
    reads = [rd([0, 1]), rd([3, 4]), rd([4, 4]), rd([1, 3])]              # known; switch (h0 | h2); skip ({4,4}: h2 walks 4, never twice in a row); skip
    species, table, hap, brk_off, rec = ref.links(WALKS, NODE_LEN, bases, reads, u64([0, 2]), np.array([0, 2], dtype=np.uint32))
    assert species.tolist() == [[4, 4, 1, 2, 1, 0]]
    assert table.tolist() == [[3, 1, 0, 0]]                                # no link is walked by both
    assert hap.tolist() == [[3, 1, 0, 2, 3, 1, 2, 1], [0] * 8]
    assert brk_off.tolist() == [0, 2, 2]
    # {1,2} at step 1: o_2 = 10 + 20; flank = min(40 // 20, 90 // 30) = 2; {2,3} at step 2: o_3 = 60; flank = min(3, 3); both masks = bit 0
    assert rec == [(1, 30, 1, 2, 2, 1), (2, 60, 2, 3, 3, 1)]
    ref.check_identities(species, table, hap, brk_off, [4, 1], u64([0, 2]))
    # one strain: private = links, no switch, core = distinct
    species, table, hap, brk_off, rec = ref.links(WALKS, NODE_LEN, bases, reads, u64([0, 1]), np.array([1], dtype=np.uint32))
    assert species.tolist() == [[4, 4, 2, 0, 0, 2]]                        # {0,1} and {1,3} are links of h1; 4 is foreign
    assert table.tolist() == [[2, 2, 2, 2]] and hap.tolist() == [[3, 3, 0, 0, 3, 3, 0, 3]]
    ref.check_identities(species, table, hap, brk_off, [4], u64([0, 1]))


def test_empty_and_skipped_by_hand():
    reads = [rd([0, 1, 2]), rd([4])]
    species, table, hap, brk_off, rec = ref.links(WALKS, NODE_LEN, BASES, reads, u64([0, 0]), np.zeros(0, dtype=np.uint32))
    assert species.tolist() == [[2, 2, 0, 0, 0, 2]] and table.tolist() == [[0, 0, 0, 0]] and hap.shape == (0, 8) and brk_off.tolist() == [0]
    ref.check_identities(species, table, hap, brk_off, [], u64([0, 0]))
    # a species of 65 selected haplotypes is skipped: the first two only
    wide = [[[0, 1]] * 65]
    species, table, hap, brk_off, rec = ref.links(wide, NODE_LEN, BASES, reads, u64([0, 65]), np.arange(65, dtype=np.uint32))
    assert species.tolist() == [[2, 2, 0, 0, 0, 0]] and not table.any() and not hap.any() and brk_off.tolist() == [0] * 66 and rec == []
    ref.check_identities(species, table, hap, brk_off, [2] * 65, u64([0, 65]))
