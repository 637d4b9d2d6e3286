"""tests/read_em_ref.py -- the row-by-row reading of the read class contract -- pinned on cases small enough to do by hand, and the host helper of the
contract (pantax_hip_read_em through pantax_amd.engine.read_em) held to it bit for bit.  No GPU."""
import numpy as np
import pytest

from tests.read_em_ref import read_classes, read_em, species_estimates

M40 = 1 << 40


def test_one_strain():
    x, n_iter, conv, delta = read_em([1], [100], [50])
    assert x.tolist() == [2.0] and (n_iter, conv, delta) == (2, 1, 0.0)


def test_two_separate_strains():
    x, n_iter, conv, delta = read_em([0b01, 0b10], [300, 70], [100, 7])
    assert x.tolist() == [3.0, 10.0] and n_iter == 2 and conv == 1 and delta <= 1e-6 * 10.0


def test_identical_strains_share_equally():
    x, n_iter, conv, _ = read_em([0b11], [600], [100, 100])                 # identical strains walk the same nodes: the same G
    assert x.tolist() == [3.0, 3.0] and conv == 1 and x[0] == 600 / (100 + 100)


def test_no_bases():
    x, n_iter, conv, delta = read_em([0b01, 0b11], [0, 0], [10, 20])
    assert x.tolist() == [0.0, 0.0] and (n_iter, conv, delta) == (2, 1, 0.0)


def test_one_iteration_is_not_convergence():
    x, n_iter, conv, delta = read_em([0b01, 0b10], [300, 70], [100, 7], max_iter=1)
    assert x.tolist() == [3.0, 10.0] and (n_iter, conv) == (1, 0) and delta == 9.0


def test_strain_without_length():
    # strain 1 has G = 0: it stays at 0, the class it holds alone gets r = 0 (every member at 0), the shared class goes to strain 0
    trace = []
    x, n_iter, conv, _ = read_em([0b01, 0b10, 0b11], [100, 55, 40], [70, 0], trace=trace)
    assert x.tolist() == [2.0, 0.0] and conv == 1 and all(t[1] == 0.0 for t in trace)


def test_floor_ends_a_dying_strain():
    # strain 1 is seen only in a class it shares with the dominant strain 0: its depth shrinks by about 100 every iteration and is cut to 0 at 1e-200
    trace = []
    x, n_iter, conv, _ = read_em([0b01, 0b11], [1000, 10], [100, 100], max_iter=300, tol=0.0, trace=trace)
    assert x[1] == 0.0 and abs(x[0] - 10.1) < 1e-12
    tail = [t[1] for t in trace if t[1] > 0.0]
    assert 50 < len(tail) < 150 and min(tail) >= 1e-200 and all(t[1] == 0.0 for t in trace[len(tail):])
    # with a tolerance the run ends long before that, the strain still positive
    x2, n2, conv2, _ = read_em([0b01, 0b11], [1000, 10], [100, 100])
    assert conv2 == 1 and n2 < 10 and 0.0 < x2[1] < 1e-6


def test_mass_is_kept():
    rng = np.random.default_rng(11)
    for _ in range(20):
        K = int(rng.integers(1, 9))
        masks = sorted(set(int(m) for m in rng.integers(1, 1 << K, size=12)))
        b = [int(v) for v in rng.integers(0, 10 ** 6, size=len(masks))]
        G = [int(v) for v in rng.integers(1, 10 ** 5, size=K)]
        x, n_iter, conv, _ = read_em(masks, b, G, max_iter=5)
        live = all(any(x[k] > 0.0 for k in range(K) if (m >> k) & 1) for m in masks)
        if live:
            assert abs(sum(x[k] * G[k] for k in range(K)) - sum(b)) <= 1e-9 * max(sum(b), 1)


def _toy():
    # one species, four haplotypes over nodes 0 .. 5
    hap_nodes = [[{0, 1, 2}, {0, 1, 3}, {0, 4}, {5}]]
    reads = [(0, True, [0], 0, 10), (0, True, [0, 1], 5, 9), (0, True, [1, 0, 1], 0, 7), (0, True, [2], 3, 1), (0, True, [4, 0], 0, 100),
             (0, True, [2, 3], 0, 50), (0, False, [0], 0, 10), (-1, True, [], 0, 10), (0, True, [0], 2, 12)]
    return hap_nodes, reads


def test_read_classes_by_hand():
    hap_nodes, reads = _toy()
    off, hap = np.array([0, 3], dtype=np.uint64), np.array([0, 1, 2], dtype=np.uint32)
    species, cls_off, mask, q = read_classes(hap_nodes, reads, off, hap)
    assert species[0, 0].tolist() == [7, 12, 181] and species[0, 1].tolist() == [1, 2, 50]      # [2, 3]: no candidate walks both
    assert cls_off.tolist() == [0, 4] and mask.tolist() == [0b001, 0b011, 0b100, 0b111]
    assert q.tolist() == [[1, 1, 0], [2, 5, 11], [1, 2, 100], [2, 2, 20]]
    # the caller's order does not enter the masks; x lands where the caller put the candidate
    hap2 = np.array([2, 0, 1], dtype=np.uint32)
    species2, cls_off2, mask2, q2 = read_classes(hap_nodes, reads, off, hap2)
    assert np.array_equal(mask2, mask) and np.array_equal(q2, q) and np.array_equal(species2, species)
    ln = np.array([30, 31, 32], dtype=np.uint64)
    x, n_iter, conv, delta = species_estimates(off, hap, ln, cls_off, mask, q)
    x2, n_iter2, conv2, delta2 = species_estimates(off, hap2, ln[[2, 0, 1]], cls_off2, mask2, q2)
    assert np.array_equal(x2.view(np.uint64), x[[2, 0, 1]].view(np.uint64)) and (n_iter2, conv2, delta2) == (n_iter, conv, delta) and x.min() > 0
    # no candidates, and more than 64: counted only
    sp0, off0, m0, _ = read_classes(hap_nodes, reads, np.array([0, 0], dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    assert sp0[0, 0].tolist() == [7, 12, 181] and not sp0[0, 1].any() and off0.tolist() == [0, 0] and len(m0) == 0
    wide = [[{0}] * 65]
    spw, offw, _, _ = read_classes(wide, [(0, True, [0], 0, 4)], np.array([0, 65], dtype=np.uint64), np.arange(65, dtype=np.uint32))
    assert spw[0, 0].tolist() == [1, 1, 4] and not spw[0, 1].any() and offw.tolist() == [0, 0]
    xw = species_estimates(np.array([0, 65], dtype=np.uint64), np.arange(65), np.ones(65), offw, np.zeros(0, dtype=np.uint64), np.zeros((0, 3), dtype=np.uint64))
    assert not xw[0].any() and xw[1][0] == 0


HAND = [([1], [100], [50], 1000, 1e-6), ([0b01, 0b10], [300, 70], [100, 7], 1000, 1e-6), ([0b11], [600], [100, 100], 1000, 1e-6),
        ([0b01, 0b11], [0, 0], [10, 20], 1000, 1e-6), ([0b01, 0b10], [300, 70], [100, 7], 1, 1e-6), ([0b01, 0b10, 0b11], [100, 55, 40], [70, 0], 1000, 1e-6),
        ([0b01, 0b11], [1000, 10], [100, 100], 300, 0.0), ([0b01, 0b11], [1000, 10], [100, 100], 1000, 1e-6), ([], [], [5, 6], 7, 0.0), ([], [], [], 3, 1e-6)]


def _random_tables():
    rng = np.random.default_rng(20261020)
    for i in range(200):
        K = int(rng.choice([1, 2, 3, 63, 64]))
        J = int(rng.integers(0, 201)) if i % 4 == 0 else int(rng.integers(0, 40))
        masks = set()
        if K <= 3:                                                          # (the zero mask may come up: a class nobody holds gets r = 0)
            masks = set(int(m) for m in rng.choice(1 << K, size=min(J, 1 << K), replace=False))
        dens = rng.uniform(0.03, 0.9)
        while K > 3 and len(masks) < J:
            m = 0
            for k in np.nonzero(rng.random(K) < dens)[0]:
                m |= 1 << int(k)
            masks.add(m)
        if i % 7 == 0:
            masks.add(0)
        masks = sorted(masks)
        top = int(rng.choice([1, 1000, M40]))
        b = [int(v) for v in rng.integers(0, top + 1, size=len(masks))]
        G = [int(v) for v in rng.integers(0, 5_000_000, size=K)]
        if i % 5 == 0:
            G[int(rng.integers(0, K))] = 0
        yield masks, b, G, int(rng.choice([1, 7, 25])), float(rng.choice([0.0, 1e-6]))


def test_host_helper_equals_the_reference_bit_for_bit():
    from pantax_amd import engine
    n, big_k, big_j, zero = 0, 0, 0, 0
    for masks, b, G, max_iter, tol in HAND + list(_random_tables()):
        ex, en, ec, ed = read_em(masks, b, G, max_iter, tol)
        gx, gn, gc, gd = engine.read_em(masks, b, G, max_iter, tol)
        assert gx.dtype == np.float64 and np.array_equal(gx.view(np.uint64), ex.view(np.uint64)), (masks[:4], b[:4], G[:4], max_iter, tol)
        assert (gn, gc) == (en, ec) and np.float64(gd).view(np.uint64) == np.float64(ed).view(np.uint64)
        n += 1
        big_k += len(G) >= 63
        big_j += len(masks) > 100
        zero += 0 in masks
    assert n == len(HAND) + 200 and big_k > 40 and big_j > 10 and zero > 10
    for bad in (([0b100], [1], [1, 1], 5, 0.0), ([1], [1], [1], 0, 0.0), ([1], [1], [1], 5, -1.0), ([1], [1], [1], 5, float("nan")), ([1], [1], [1], 5, float("inf"))):
        with pytest.raises(ValueError):
            engine.read_em(*bad)
    with pytest.raises(ValueError):
        engine.read_em([1], [1], [1] * 65)
