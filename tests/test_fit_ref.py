"""Pins tests/fit_ref.py, the numpy restatement of the pantax_hip_strain_fit contract the GPU tests compare against, on a case computed by hand:
ties that round to even in both directions, a clamped E, a sum whose value depends on the order of its additions, and the identities of the contract."""
from types import SimpleNamespace

import numpy as np

from tests.fit_ref import E_MAX, check_identities, expected_bases, fit


def _graph(node_len, walks):
    off = np.concatenate([[0], np.cumsum([len(w) for w in walks])]).astype(np.uint64)
    return SimpleNamespace(node_len=np.array(node_len, dtype=np.uint32), path_off=off, path_nodes=np.array([v for w in walks for v in w], dtype=np.uint32),
                           n_paths=len(walks))


# species 0: the selection [2, 0, 1] in an order that is not the index order; haplotype 3 is not selected (its nodes 4, 5 are orphans)
S0 = _graph([1, 3, 5, 1, 4, 2, 5], [[0, 1, 0], [0, 2], [0, 1, 3, 6], [4, 5]])
B0 = [1, 0, 9, 0, 7, 3, 4]
# species 1: one strain at 1e18 (exact in f64): t = 1e19 >= 2^62 on node 0, t = 2e18 < 2^62 on node 1;  species 2: nothing selected
S1 = _graph([10, 2], [[0, 1]])
B1 = [5, 1 << 40]
S2 = _graph([3], [[0]])
B2 = [4]
SEL_OFF = np.array([0, 3, 4, 4], dtype=np.uint64)
SEL_HAP = np.array([2, 0, 1, 0], dtype=np.uint32)
SEL_W = np.array([0.5, 2.0 ** -54, 2.0 ** -54, 1e18], dtype=np.float64)
BASES = np.array(B0 + B1 + B2, dtype=np.uint64)


def test_order_of_the_sum_in_plain_f64():
    """what the case rests on: ascending index gives 0.5 + 2^-53, the list order gives 0.5"""
    a, h = np.float64(2.0 ** -54), np.float64(0.5)
    assert (a + a) + h == np.float64(0.5 + 2.0 ** -53) and (a + a) + h > h
    assert (h + a) + a == h
    assert expected_bases([(a + a) + h, (h + a) + a], [1, 1]).tolist() == [1, 0]


def test_rounding_and_clamps():
    assert expected_bases([0.5, 0.5, 0.5, 0.5, 0.25], [1, 3, 5, 7, 2]).tolist() == [0, 2, 2, 4, 0]           # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4 (ties), 0.5 -> 0
    assert expected_bases([0.0, 1.0, 2.0 ** 62, 2.0 ** 61, 1e300, np.inf, np.inf], [5, 0, 1, 1, 7, 1, 0]).tolist() == [0, 0, E_MAX, 1 << 61, E_MAX, E_MAX, 0]
    assert expected_bases([np.nextafter(2.0 ** 62, 0)], [1]).tolist() == [(1 << 62) - 512]                    # the largest t below the clamp: an integer already


def test_hand_computed_case():
    hap, sp = fit([S0, S1, S2], SEL_OFF, SEL_HAP, SEL_W, BASES)
    assert hap.dtype == sp.dtype == np.uint64 and hap.shape == (4, 2, 8) and sp.shape == (3, 3, 8)
    # species 0, node by node (n, len, b, E, excess, deficit, blind, blind_E):
    #   v0 M = {0, 1, 2}: p = (2^-54 + 2^-54) + 0.5 = 0.5 + 2^-53, len 1 -> E = 1 (list order would give 0.5 -> 0);  b = 1            (1, 1, 1, 1, 0, 0, 0, 0)
    #   v1 M = {0, 2}: p = 2^-54 + 0.5 = 0.5 (a tie, to even), len 3 -> t = 1.5 -> E = 2;  b = 0: blind                               (1, 3, 0, 2, 0, 2, 1, 2)
    #   v2 M = {1}: p = 2^-54, len 5 -> E = 0;  b = 9                                                                               (1, 5, 9, 0, 9, 0, 0, 0)
    #   v3 M = {2}: p = 0.5, len 1 -> t = 0.5 -> E = 0;  b = 0 and E = 0: not blind                                                 (1, 1, 0, 0, 0, 0, 0, 0)
    #   v4, v5 orphans: E = 0, excess = b                                                                    (1, 4, 7, 0, 7, 0, 0, 0), (1, 2, 3, 0, 3, 0, 0, 0)
    #   v6 M = {2}: p = 0.5, len 5 -> t = 2.5 -> E = 2;  b = 4                                                                      (1, 5, 4, 2, 2, 0, 0, 0)
    assert hap[0].tolist() == [[4, 10, 5, 5, 2, 2, 1, 2], [2, 6, 4, 2, 2, 0, 0, 0]]          # haplotype 2: all = v0 v1 v3 v6, private = v3 v6
    assert hap[1].tolist() == [[2, 4, 1, 3, 0, 2, 1, 2], [0] * 8]                            # haplotype 0 (its walk visits node 0 twice): v0 v1, nothing private
    assert hap[2].tolist() == [[2, 6, 10, 1, 9, 0, 0, 0], [1, 5, 9, 0, 9, 0, 0, 0]]          # haplotype 1: v0 v2, private v2
    assert sp[0].tolist() == [[7, 21, 24, 5, 21, 2, 1, 2], [5, 15, 14, 5, 11, 2, 1, 2], [2, 6, 10, 0, 10, 0, 0, 0]]
    # species 1: K = 1 -> all == private == explained; node 0 clamped
    e0, e1 = E_MAX, 2 * 10 ** 18
    one = [2, 12, 5 + (1 << 40), e0 + e1, 0, (e0 - 5) + (e1 - (1 << 40)), 0, 0]
    assert hap[3].tolist() == [one, one] and sp[1].tolist() == [one, one, [0] * 8]
    # species 2: nothing selected -> total == orphan, nothing expected
    assert sp[2].tolist() == [[1, 3, 4, 0, 4, 0, 0, 0], [0] * 8, [1, 3, 4, 0, 4, 0, 0, 0]]
    check_identities(hap, sp)


def test_selection_order_does_not_matter_and_zero_weights():
    hap, sp = fit([S0, S1, S2], SEL_OFF, SEL_HAP, SEL_W, BASES)
    perm = [1, 2, 0, 3]                                                  # the same selection listed as [0, 1, 2]
    hap2, sp2 = fit([S0, S1, S2], SEL_OFF, SEL_HAP[perm], SEL_W[perm], BASES)
    assert np.array_equal(hap2, hap[perm]) and np.array_equal(sp2, sp)
    hap0, sp0 = fit([S0, S1, S2], SEL_OFF, SEL_HAP, np.zeros(4), BASES)  # all weights zero: nothing expected, nothing blind
    assert not hap0[:, :, 3].any() and not hap0[:, :, 5:].any() and not sp0[:, :, 3].any() and not sp0[:, :, 5:].any()
    assert np.array_equal(hap0[:, :, :3], hap[:, :, :3]) and np.array_equal(hap0[:, :, 4], hap0[:, :, 2])
    check_identities(hap0, sp0)
