"""The reference of the fragment support (tests/fragments_ref.py) pinned by hand: the key and tag of crafted ids, the mates of crafted keys (seen once,
twice with every tag pair, three and four times), and a species of three strains whose reads fall into every class, counted on paper."""
import numpy as np
import pytest

from tests import fragments_ref as ref
from tests.helpers import gaf_id_hash

NONE, AMB = ref.MATE_NONE, ref.MATE_AMBIGUOUS


def test_key_and_tag_of_crafted_ids():
    h = gaf_id_hash
    assert ref.fragment_key(b"a/1") == (h(b"a"), 1)                  # exactly 3 bytes: the shortest id with a suffix
    assert ref.fragment_key(b"a/2") == (h(b"a"), 2)
    assert ref.fragment_key(b"/1") == (h(b"/1"), 0)                  # no stem: the whole id
    assert ref.fragment_key(b"x/3") == (h(b"x/3"), 0)
    assert ref.fragment_key(b"ab") == (h(b"ab"), 0)
    assert ref.fragment_key(b"a/") == (h(b"a/"), 0)
    assert ref.fragment_key(b"") == (h(b""), 0)
    assert ref.fragment_key(b"S0R4970856/2") == (h(b"S0R4970856"), 2)
    assert ref.fragment_key(b"a/1/1") == (h(b"a/1"), 1)              # only the last suffix is cut
    assert ref.fragment_key(b"a") == (h(b"a"), 0)                    # the bare stem has the key of its two suffixed mates


def test_mates_of_crafted_keys():
    #       0   1   2   3   4   5   6   7   8   9  10  11  12  13  14  15  16  17  18  19  20
    key = [10, 11, 10, 12, 13, 12, 14, 14, 15, 15, 16, 16, 17, 17, 18, 18, 18, 19, 19, 19, 19]
    tag = [1,  0,  2,  0,  2,  0,  2,  1,  1,  1,  2,  2,  0,  1,  1,  2,  0,  0,  0,  0,  0]
    mate, counts = ref.fragment_mates(key, tag)
    assert mate.dtype == np.uint32 and counts.dtype == np.uint64
    assert mate.tolist() == [2, NONE, 0, 5, NONE, 3, 7, 6, AMB, AMB, AMB, AMB, AMB, AMB, AMB, AMB, AMB, AMB, AMB, AMB, AMB]
    # pairs: 10 {1,2}, 12 {0,0}, 14 {2,1}; none: 11, 13; ambiguous reads: 15 {1,1}, 16 {2,2}, 17 {0,1}, 18 x3, 19 x4; crowded keys: 18, 19
    assert counts.tolist() == [3, 2, 13, 2]
    good = {(0, 0), (1, 2), (2, 1)}
    for a in range(3):                                                        # all nine tag pairs of a twice-seen key
        for b in range(3):
            mate2, counts2 = ref.fragment_mates([5, 5], [a, b])
            assert mate2.tolist() == ([1, 0] if (a, b) in good else [AMB, AMB])
            assert counts2.tolist() == ([1, 0, 0, 0] if (a, b) in good else [0, 0, 2, 0])
    m0, c0 = ref.fragment_mates([], [])
    assert len(m0) == 0 and c0.tolist() == [0, 0, 0, 0]
    assert ref.fragment_mates([7], [1])[0].tolist() == [NONE]
    assert ref.check_mates(mate) and ref.check_mates([])
    assert not ref.check_mates([1, NONE]) and not ref.check_mates([0]) and not ref.check_mates([5, 0]) and not ref.check_mates([1, 2, 0])


# one species of three strains over nodes 0 .. 7, a second of K_s = 0, a third that is skipped (K_s = 65 is built below)
#   A walks {0, 1, 2, 3}      B walks {0, 1, 4, 5}      C walks {0, 4, 6}          node 7: nobody
HAPS = [[{0, 1, 2, 3}, {0, 1, 4, 5}, {0, 4, 6}], [{0, 1}], [{0}] * 65]
CAND_OFF = np.array([0, 3, 3, 68], dtype=np.uint64)
CAND_HAP = np.array([2, 0, 1] + list(range(65)), dtype=np.uint32)             # entries of species 0: C, A, B (any order)
CAND_W = np.array([5.0, 1.0, 5.0] + [1.0] * 65)                               # B and C tie: the smaller haplotype index (B) is assigned


def _reads():
    R = lambda s, nodes, counted=True, ps=10, pe=30: (s, counted, nodes, ps, pe)
    rows = [
        R(0, [0]), R(0, [0, 1]),            # 0, 1   concordant: C = {A,B,C} and {A,B}, F = {A,B}: assigned B (weight 5 over 1)
        R(0, [0, 1]), R(0, [0, 4]),         # 2, 3   unique_by_pair: {A,B} and {B,C}, F = {B}
        R(0, [2]), R(0, [1]),               # 4, 5   unique, not by pair: {A} and {A,B}, F = {A}
        R(0, [2]), R(0, [6]),               # 6, 7   discordant: {A} and {C}, filed at (A, C)
        R(0, [7]), R(0, [0]),               # 8, 9   half: {} and {A,B,C}
        R(0, [7]), R(0, [2, 4]),            # 10, 11 unexplained: {} and {}
        R(0, [0], ps=30, pe=10),            # 12     single; span 0 (pend < pstart)
        R(0, [0]), R(0, [0]), R(0, [0]),    # 13..15 multi (a key seen three times)
        R(0, [0]), R(0, [0], counted=False),   # 16, 17 the mate is dropped by its flags
        R(0, [1]), R(-1, []),               # 18, 19 the mate has no walk
        R(0, [1]), R(1, [0, 1]),            # 20, 21 the mate sits in another species; 21 is of the K_s = 0 species
        R(1, [0]), R(1, [1, 0, 1]),         # 22, 23 paired in the K_s = 0 species
        R(2, [0]), R(2, [0]),               # 24, 25 paired in the skipped species
        R(0, [0, 4], ps=0, pe=7), R(0, [4], ps=1, pe=3),   # 26, 27 concordant, F = {B,C}: the tie goes to B
    ]
    mate = [1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10, NONE, AMB, AMB, AMB, 17, 16, 19, 18, 21, 20, 23, 22, 25, 24, 27, 26]
    return rows, np.array(mate, dtype=np.uint32)


def test_fragment_pass_by_hand():
    rows, mate = _reads()
    hap, species, status, pair_off, pair, n = ref.strain_fragments(HAPS, rows, CAND_OFF, CAND_HAP, CAND_W, mate)
    assert status.tolist() == [0, 1, ref.E_LIMIT] and pair_off.tolist() == [0, 9, 9, 9]
    sp = species[0]
    assert sp[ref.COUNTED].tolist() == [21, 26, 18 * 20 + 7 + 2]            # reads 0..16, 18, 20, 26, 27; read 12 spans 0
    assert sp[ref.PAIRED].tolist() == [7, 3 + 4 + 2 + 2 + 2 + 3 + 3, 6 * 40 + 9]
    assert sp[ref.CONCORDANT].tolist() == [4, 3 + 4 + 2 + 3, 3 * 40 + 9]
    assert sp[ref.DISCORDANT].tolist() == [1, 2, 40] and sp[ref.HALF].tolist() == [1, 2, 40] and sp[ref.UNEXPLAINED].tolist() == [1, 3, 40]
    assert sp[ref.SINGLE].tolist() == [1, 1, 0] and sp[ref.MULTI].tolist() == [3, 3, 60] and sp[ref.ELSEWHERE].tolist() == [3, 3, 60]
    C_, A_, B_ = 0, 1, 2                                                     # the entries, in the caller's order
    assert hap[A_, ref.COMPATIBLE].tolist() == [2, 3 + 2, 80] and hap[B_, ref.COMPATIBLE].tolist() == [3, 3 + 4 + 3, 89] and hap[C_, ref.COMPATIBLE].tolist() == [1, 3, 9]
    assert hap[A_, ref.UNIQUE].tolist() == [1, 2, 40] and hap[B_, ref.UNIQUE].tolist() == [1, 4, 40] and not hap[C_, ref.UNIQUE].any()
    assert hap[B_, ref.UNIQUE_BY_PAIR].tolist() == [1, 4, 40] and not hap[A_, ref.UNIQUE_BY_PAIR].any() and not hap[C_, ref.UNIQUE_BY_PAIR].any()
    assert hap[A_, ref.ASSIGNED].tolist() == [1, 2, 40] and hap[B_, ref.ASSIGNED].tolist() == [3, 10, 89] and not hap[C_, ref.ASSIGNED].any()
    m = pair[0:9].reshape(3, 3)
    assert m[A_, C_] == 1 and m[C_, A_] == 1 and m.sum() == 2
    assert species[1, ref.COUNTED].tolist() == [3, 6, 60] and species[1, ref.PAIRED].tolist() == [1, 4, 40] and species[1, ref.ELSEWHERE].tolist() == [1, 2, 20]
    assert not species[1, ref.CONCORDANT:ref.UNEXPLAINED + 1].any() and not species[1, ref.SINGLE].any()
    assert species[2, ref.COUNTED].tolist() == [2, 2, 40] and species[2, ref.PAIRED].tolist() == [1, 2, 40] and not species[2, 2:].any() and not hap[3:].any()
    assert n.tolist() == [2, 2, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, -1, -1, -1, -1, -1, -1, -1, -2, -1, -1, -1, -1, -1, -1, 2, 2]
    ref.check_identities(hap, species, status, pair_off, pair, CAND_OFF)
    from tests.read_support_ref import read_support
    ref.check_identities(hap, species, status, pair_off, pair, CAND_OFF, read_support(HAPS, rows, CAND_OFF, CAND_HAP, CAND_W)[1])


def test_all_none_is_single():
    rows, mate = _reads()
    hap, species, status, pair_off, pair, n = ref.strain_fragments(HAPS, rows, CAND_OFF, CAND_HAP, CAND_W, np.full(len(rows), NONE, dtype=np.uint32))
    assert np.array_equal(species[:, ref.SINGLE], species[:, ref.COUNTED]) and species[:, ref.COUNTED, 0].tolist() == [21, 3, 2]
    assert not species[:, ref.PAIRED:ref.UNEXPLAINED + 1].any() and not species[:, ref.MULTI:].any() and not hap.any() and not pair.any()
    assert set(n.tolist()) == {-1, -2}


def test_invalid_mates_are_refused():
    rows, mate = _reads()
    for r, v in ((0, 2), (0, 0), (0, len(rows)), (12, 0)):                   # asymmetric, self, out of range, a single named by nobody
        bad = mate.copy()
        bad[r] = v
        with pytest.raises(ValueError):
            ref.strain_fragments(HAPS, rows, CAND_OFF, CAND_HAP, CAND_W, bad)
