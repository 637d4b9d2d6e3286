"""The plain-Python reading of the mosaic read contract (tests/mosaic_ref.py) pinned by hand: small cases with every expected number written out, the
greedy cut against a brute-force minimum over all cuts and against the reversed walk, the identities against tests/read_support_ref.py on random inputs,
and the host helpers of the library (pantax_hip_mosaic_walk, pantax_hip_mosaic_top; no GPU) against the reference."""
import itertools
import random

import numpy as np
import pytest

from tests import mosaic_ref as ref
from tests.read_support_ref import read_support

# one species, three candidates (entries 0, 1, 2 = haplotypes 0, 1, 2): nodes 0-3 are walked by 0 and 1, 4-7 by 1 and 2, 8 by 0 alone, 9 by nobody
HAP3 = [[{0, 1, 2, 3, 8}, {0, 1, 2, 3, 4, 5, 6, 7}, {4, 5, 6, 7}]]
OFF3 = np.array([0, 3], dtype=np.uint64)
CH3 = np.array([0, 1, 2], dtype=np.uint32)


def _run(nodes, w=(1.0, 2.0, 3.0), hap_nodes=HAP3, off=OFF3, ch=CH3, pstart=10, pend=50, counted=True):
    return ref.mosaic(hap_nodes, [(0, counted, nodes, pstart, pend)], off, ch, np.array(w, dtype=np.float64))


def test_one_break():
    # 8 is walked by candidate 0 only, 4 and 5 by 1 and 2: {0} then {1, 2}; the right segment goes to the heavier candidate 2
    species, extra, hap, pair_off, pair, jn, jc, total = _run([0, 8, 4, 5])
    assert species[0].tolist() == [[1, 4, 40], [0, 0, 0], [1, 4, 40], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert extra[0].tolist() == [2, 1, 0]
    assert hap.tolist() == [[1, 2], [0, 0], [1, 2]]
    assert pair_off.tolist() == [0, 9] and pair.reshape(3, 3).tolist() == [[0, 0, 1], [0, 0, 0], [0, 0, 0]]
    assert jn.tolist() == [[0, 8, 4]] and jc.tolist() == [1] and total == 1


def test_break_at_the_first_possible_step():
    # the second step already empties the intersection: segments of one step and of two
    species, extra, hap, pair_off, pair, jn, jc, total = _run([8, 4, 5])
    assert species[0, ref.MOSAIC1].tolist() == [1, 3, 40] and extra[0].tolist() == [2, 1, 0]
    assert hap.tolist() == [[1, 1], [0, 0], [1, 2]] and jn.tolist() == [[0, 8, 4]]
    # the break goes as late as it can: 0 1 2 3 fit candidate 1 together with 4, so the cut {0,1} | {1,2} is not taken -- one read, compatible
    species, extra, hap, _, pair, jn, _, total = _run([0, 1, 4, 5])
    assert species[0, ref.COMPATIBLE].tolist() == [1, 4, 40] and not extra.any() and not hap.any() and not pair.any() and total == 0 and len(jn) == 0


def test_foreign_step_before_and_after_a_would_be_break():
    for nodes, n_foreign in (([9, 8, 4], 1), ([8, 4, 9], 1), ([9, 8, 4, 9, 9], 3)):
        species, extra, hap, _, pair, jn, _, total = _run(nodes)
        assert species[0, ref.FOREIGN].tolist() == [1, len(nodes), 40] and species[0, ref.COUNTED].tolist() == [1, len(nodes), 40]
        assert not species[0, 1:5].any() and extra[0].tolist() == [0, 0, n_foreign]
        assert not hap.any() and not pair.any() and total == 0 and len(jn) == 0      # not cut: no segments, switches or junctions


def test_node_visited_twice_across_a_break():
    # 8 | 4 5 | 8: node 8 on both sides, three segments, the junctions (8, 4) and (5, 8); weights make candidate 1 win the middle
    species, extra, hap, _, pair, jn, jc, total = _run([8, 4, 5, 8], w=(1.0, 5.0, 3.0))
    assert species[0, ref.MOSAIC2].tolist() == [1, 4, 40] and extra[0].tolist() == [3, 2, 0]
    assert hap.tolist() == [[2, 2], [1, 2], [0, 0]]
    assert pair.reshape(3, 3).tolist() == [[0, 1, 0], [1, 0, 0], [0, 0, 0]]          # [a][b] and [b][a]: walk order, not mirrored
    assert jn.tolist() == [[0, 5, 8], [0, 8, 4]] and jc.tolist() == [1, 1] and total == 2
    # k = 4: mosaic3plus
    species, extra, *_ = _run([8, 4, 8, 4])
    assert species[0, ref.MOSAIC3PLUS].tolist() == [1, 4, 40] and extra[0].tolist() == [4, 3, 0]


def test_equal_weights_go_to_the_smallest_haplotype():
    # candidates given in the order 2, 0, 1: entry 0 is haplotype 2.  {1, 2} with equal weights is assigned haplotype 1 = entry 2
    ch = np.array([2, 0, 1], dtype=np.uint32)
    species, extra, hap, _, pair, jn, _, _ = _run([8, 4, 5], w=(3.0, 3.0, 3.0), ch=ch)
    assert hap.tolist() == [[0, 0], [1, 1], [1, 2]]                                   # entry 1 = haplotype 0 (left), entry 2 = haplotype 1 (right)
    assert pair.reshape(3, 3).tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 0]]          # positions in the caller's order


def test_k_0_1_65_and_dropped_reads():
    # K_s = 0: counted only
    species, extra, hap, pair_off, pair, jn, jc, total = ref.mosaic(HAP3, [(0, True, [8, 4], 0, 7)], np.array([0, 0], dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0))
    assert species[0].tolist() == [[1, 2, 7]] + [[0, 0, 0]] * 5 and not extra.any() and pair_off.tolist() == [0, 0] and total == 0
    # K_s = 1: compatible or foreign, never mosaic
    one = (np.array([0, 1], dtype=np.uint64), np.array([0], dtype=np.uint32), np.array([1.0]))
    species, extra, hap, pair_off, pair, jn, jc, total = ref.mosaic(HAP3, [(0, True, [0, 8], 0, 7), (0, True, [8, 4], 9, 3)], *one)
    assert species[0].tolist() == [[2, 4, 7], [1, 2, 7], [0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 2, 0]] and extra[0].tolist() == [0, 0, 1]
    assert not hap.any() and pair.tolist() == [0] and total == 0
    # K_s = 65: counted only, no pair block
    wide = [[{h, 100} for h in range(65)]]
    off = np.array([0, 65], dtype=np.uint64)
    species, extra, hap, pair_off, pair, jn, jc, total = ref.mosaic(wide, [(0, True, [0, 1], 0, 7)], off, np.arange(65, dtype=np.uint32), np.ones(65))
    assert species[0].tolist() == [[1, 2, 7]] + [[0, 0, 0]] * 5 and not extra.any() and not hap.any() and pair_off.tolist() == [0, 0] and total == 0
    # a dropped read and a read of no species count nowhere
    species, *_ = ref.mosaic(HAP3, [(0, False, [8, 4], 0, 7), (-1, True, [], 0, 7)], OFF3, CH3, np.ones(3))
    assert not species.any()


def _brute_min(member):
    """the smallest number of stretches that each have a common candidate, over all cuts"""
    n = len(member)
    for k in range(1, n + 1):
        for cuts in itertools.combinations(range(1, n), k - 1):
            b = (0,) + cuts + (n,)
            if all(set.intersection(*member[b[i]:b[i + 1]]) for i in range(k)):
                return k
    raise AssertionError("a walk without empty steps can be cut into single steps")


def test_greedy_is_minimal_and_direction_free():
    rng = random.Random(11)
    seen = set()
    for _ in range(400):
        K = rng.randint(1, 5)
        n = rng.randint(1, 9)
        member = [set(c for c in range(K) if rng.random() < 0.6) or {rng.randrange(K)} for _ in range(n)]
        k = len(ref.cut(member))
        assert k == _brute_min(member) == len(ref.cut(member[::-1]))
        seen.add(min(k, 4))
    assert seen == {1, 2, 3, 4}


def _random_world(rng):
    S = 3
    n_nodes = 14
    hap_nodes = [[set(v for v in range(n_nodes) if rng.random() < 0.55) for _ in range(rng.randint(1, 5))] for _ in range(S)]
    picks = [sorted(rng.sample(range(len(h)), rng.randint(0, len(h)))) for h in hap_nodes]
    for p in picks:
        rng.shuffle(p)
    off = np.cumsum([0] + [len(p) for p in picks]).astype(np.uint64)
    ch = np.array(sum(picks, []), dtype=np.uint32)
    cw = np.array([rng.choice([1.0, 2.0, 2.0, 3.5]) for _ in ch], dtype=np.float64)
    reads = []
    for _ in range(120):
        s = rng.randrange(-1, S)
        nodes = [rng.randrange(n_nodes) for _ in range(rng.randint(1, 7))]
        if s >= 0 and hap_nodes[s] and rng.random() < 0.7:                            # mostly stretches of real walks, so that not every read is foreign
            nodes = [rng.choice(sorted(rng.choice(hap_nodes[s])) or [0]) for _ in nodes]
        reads.append((s, rng.random() < 0.9, nodes, rng.randrange(50), rng.randrange(50)))
    return hap_nodes, reads, off, ch, cw


def test_identities_against_read_support_reference():
    rng = random.Random(5)
    tot = np.zeros(6, dtype=np.int64)
    for _ in range(30):
        hap_nodes, reads, off, ch, cw = _random_world(rng)
        out = ref.mosaic(hap_nodes, reads, off, ch, cw)
        sup = read_support(hap_nodes, reads, off, ch, cw)
        ref.check_identities(*out[:7], off, support_species=sup[1])
        assert out[7] == int(out[1][:, ref.N_BREAKS].sum()) == int(out[6].sum())
        tot += out[0][:, :, 0].sum(axis=0).astype(np.int64)
    assert (tot > 0).all()                                                            # every class occurred


# ---- the host helpers of the library: no GPU ----------------------------------------------------------------------------------------------

def _masks(member, K):
    return np.array([sum(1 << c for c in m) for m in member], dtype=np.uint64)


def test_library_mosaic_walk_equals_reference():
    from pantax_amd import engine
    rng = random.Random(3)
    for _ in range(300):
        K = rng.choice([1, 2, 3, 5, 64])
        n = rng.randint(0, 12)
        member = [set(c for c in range(K) if rng.random() < (0.5 if K < 64 else 0.05)) for _ in range(n)]
        if rng.random() < 0.7:
            member = [m or {rng.randrange(K)} for m in member]
        hap = np.array(rng.sample(range(K + 3), K), dtype=np.uint32)
        w = np.array([rng.choice([1.0, 2.0, 2.0]) for _ in range(K)], dtype=np.float64)
        k, fs, seg_end, seg_pos = engine.mosaic_walk(_masks(member, K), w, hap)
        empty = sum(1 for m in member if not m)
        assert fs == empty
        if empty or n == 0:
            assert k == 0
            continue
        segs = ref.cut(member)
        assert k == len(segs) and seg_end.tolist() == [b for _, b, _ in segs]
        assert seg_pos.tolist() == [ref.assigned(A, hap, w) for _, _, A in segs]
    with pytest.raises(ValueError):
        engine.mosaic_walk(np.array([1, 2, 1], dtype=np.uint64), np.ones(2), np.array([0, 1], dtype=np.uint32), cap=2)    # k = 3 > cap
    with pytest.raises(ValueError):
        engine.mosaic_walk(np.array([1], dtype=np.uint64), np.ones(2), np.array([4, 4], dtype=np.uint32))                   # a haplotype twice
    with pytest.raises(ValueError):
        engine.mosaic_walk(np.array([1], dtype=np.uint64), np.ones(65), np.arange(65, dtype=np.uint32))                     # K > 64


def test_library_mosaic_top_equals_reference():
    from pantax_amd import engine
    rng = random.Random(9)
    for _ in range(100):
        n = rng.randint(0, 30)
        keys = sorted(set((0, rng.randrange(6), rng.randrange(6)) for _ in range(n)))
        jn = np.array(keys, dtype=np.uint32).reshape(len(keys), 3)
        jc = np.array([rng.randint(1, 4) for _ in keys], dtype=np.uint64)
        for top in (0, 1, 3, 100):
            assert engine.mosaic_top(jn[:, 1], jn[:, 2], jc, top).tolist() == ref.top(jn, jc, 0, top)
