"""The plain-Python reference of the rarefaction of the strain fit (tests/rarefy_ref.py) on a case done by hand, the library's host helper
pantax_hip_rarefy_depth against it over a few thousand (seed, replicate, read) with reads at and beyond 2^32, and the nestedness of the levels.  No GPU."""
import numpy as np
import pytest

from tests import bootstrap_ref as bref
from tests import rarefy_ref as ref


def _case():
    import synthdata as synth
    node_len = np.array([10, 20, 30], dtype=np.int64)
    paths = [[0, 1, 2], [0, 2]]
    off = np.array([0, 3, 5], dtype=np.uint64)
    g = synth.SpeciesGraph("77", node_len, off, np.concatenate(paths).astype(np.uint32), ["h0", "h1"], 1, 3, np.array([60, 40], dtype=np.int64), np.ones(2))
    walks = [[1, 2, 3], [1], [2, 3], [3, 3], [1, 2]]
    ps = [0, 2, 5, 0, 11]
    pe = [60, 7, 30, 60, 40]
    so = np.concatenate([[0], np.cumsum([len(w) for w in walks])]).astype(np.uint64)
    n = len(walks)
    reads = synth.PackedReads(so, np.concatenate(walks).astype(np.uint32), np.zeros(int(so[-1]), np.uint8), np.array(ps, dtype=np.int64), np.array(pe, dtype=np.int64),
                              np.full(n, 150, np.int64), np.full(n, 60, np.int64), np.zeros(n, np.int64))
    return g, reads


def test_reference_on_a_hand_computed_case():
    g, reads = _case()
    # read 0 covers the three nodes whole; read 1 is a one-node read of 5 bases; read 2 adds 20 - 5 and then target 25 - 15 = 10; read 3 walks node 2 twice:
    # the first occurrence alone adds its 30; read 4 starts beyond its first node: an abort, nothing
    assert ref.species_bases(g, reads, np.ones(5, dtype=bool)).tolist() == [15, 35, 70]
    assert ref.species_bases(g, reads, np.array([1, 2])).tolist() == [5, 15, 10]
    assert ref.species_bases(g, reads, np.array([4])).tolist() == [0, 0, 0]
    mask, a = ref.entry_rows(g, np.array([15, 35, 70]), np.array([0, 1]))
    assert mask.tolist() == [1, 3, 3] and a.tolist() == [35 / 20, 15 / 10, 70 / 30]
    assert ref.member_counts(mask, 2).tolist() == [[3, 1], [2, 0]]
    mask, a = ref.entry_rows(g, np.array([15, 35, 70]), np.array([1, 0]))     # the columns follow the selection's order
    assert mask.tolist() == [2, 3, 3] and ref.member_counts(mask, 2).tolist() == [[2, 0], [3, 1]]
    mask, a = ref.entry_rows(g, np.array([0, 35, 0]), np.array([1]))          # the one covered node has no member: no row
    assert len(a) == 0
    # the stage reference from the depths of the rule: every level's bases are those of its kept reads
    sp = np.zeros(5, dtype=np.int32)
    counted = np.array([True, True, True, False, True])                      # read 3 carries a drop flag
    seed, L, B = 5, 3, 4
    out = ref.stage_reference([g], reads, sp, counted, [0, 2], [0, 1], seed, L, B)
    assert len(out) == 1 + L * B and out[0][0]["reads"] == [4, 15 + 35 + 40] and out[0][0]["n_rows"] == 3
    full = [np.array(x) for x in ([10, 20, 30], [5, 0, 0], [0, 15, 10], [0, 0, 30], [0, 0, 0])]
    seen = set()
    for b in range(1, B + 1):
        d = ref.depths(seed, b, 5)
        for level in range(1, L + 1):
            keep = [r for r in range(5) if counted[r] and d[r] >= level]
            bases = sum((full[r] for r in keep), np.zeros(3, dtype=np.int64))
            rec = out[ref.entry(L, b, level)][0]
            assert rec["reads"] == [len(keep), int(bases.sum())]
            assert rec["n_rows"] == int((bases > 0).sum()) and rec["status"] == (0 if bases.any() else 1)
            seen.add(len(keep))
    assert len(seen) > 1
    # the rows of the report: level 0 is entry 0 alone, scaled_mean = mean x 2^level, max beside the summary's min
    E = 1 + 2 * 2
    x = [3.0, 1.0, 0.0, 2.0, 0.5]                                             # entry 0; (b 1, l 1), (b 1, l 2), (b 2, l 1), (b 2, l 2)
    status = [0, 0, 0, 0, 1]
    member = [[7, 1], [4, 0], [2, 0], [6, 2], [0, 0]]
    rows = ref.strain_rows(["77", "t", "g"], 2.5, x, status, member, 2, 2)
    assert len(rows) == 3 and all(len(r) == len(ref.HEADER) == 21 for r in rows)
    assert rows[0][3:] == ["strain", 0, 1.0, 1, 2.5, 3.0, 3.0, 0.0, 3.0, 3.0, 3.0, 0.0, 7.0, 1.0, "-", "-", "-", "-"]
    assert rows[1][3:] == ["strain", 1, 0.5, 2, 2.5, 3.0, 1.5, np.sqrt(0.5), 1.0, 2.0, 3.0, 0.0, 5.0, 1.0, "-", "-", "-", "-"]
    assert rows[2][3:] == ["strain", 2, 0.25, 1, 2.5, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, "-", "-", "-", "-"]
    srows = ref.species_rows(["77"], [9.0, 4.0, 1.0, 2.0, 0.0], status, [30, 20, 8, 10, 0], [[100, 5000], [50, 2500], [20, 900], [60, 3100], [0, 0]], 2, 2)
    assert srows[1] == ["77", "-", "-", "species", 1, 0.5, 2] + ["-"] * 10 + [55.0, 2800.0, 15.0, 3.0]
    assert srows[2] == ["77", "-", "-", "species", 2, 0.25, 1] + ["-"] * 10 + [10.0, 450.0, 4.0, 1.0]
    assert len(ref.skipped_row(["77"])) == 21
    assert ref.parse_row(["a", "b", "c", "strain", "2", "0.25", "1", "2.5", "-"]) == ["a", "b", "c", "strain", 2, 0.25, 1, 2.5, "-"]


def _depth_np(seed, b, r):
    """the rule once more, on numpy's wrapping uint64 arithmetic (bootstrap_ref._sm_np) and a count of leading zeros by shifting"""
    one = lambda v: bref._sm_np(np.array([v], dtype=np.uint64))[0]
    with np.errstate(over="ignore"):
        h = int(one(one(np.uint64(seed) ^ one(np.uint64(b))) + np.uint64(r)))
    z = 0
    while z < 64 and not (h >> (63 - z)) & 1:
        z += 1
    return min(z, 63)


def test_depth_rule_and_host_helper():
    assert bref.sm(0) == 0xE220A8397B1DCDAF                                   # splitmix64's first output from state 0
    from pantax_amd.engine import rarefy_depth
    rng = np.random.default_rng(11)
    cases = [(42, 1, 0), (42, 1, 1), (0, 1, 0), (0, 0, 0), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 64 - 1), (7, 3, 2 ** 32), (7, 3, 2 ** 32 + 1), (7, 3, 2 ** 40 + 5)]
    for _ in range(3000):
        cases.append((int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(0, 2 ** 32)),
                      int(rng.integers(0, 2 ** 63)) if rng.integers(0, 2) else int(rng.integers(0, 5000))))
    hist = np.zeros(64, dtype=np.int64)
    for seed, b, r in cases:
        d = ref.depth(seed, b, r)
        assert 0 <= d <= 63 and rarefy_depth(seed, b, r) == d, (seed, b, r)
        hist[d] += 1
    for seed, b, r in cases[:300]:
        assert _depth_np(seed, b, r) == ref.depth(seed, b, r)
    assert any(r >= 2 ** 32 for _, _, r in cases) and 0.4 < hist[0] / len(cases) < 0.6 and 0.18 < hist[1] / len(cases) < 0.32
    # a run of reads of one replicate: the read index matters beyond 32 bits, the replicate and the seed matter
    a = [rarefy_depth(9, 2, r) for r in range(2000)]
    assert a != [rarefy_depth(9, 2, r + 2 ** 32) for r in range(2000)] and a != [rarefy_depth(9, 3, r) for r in range(2000)] and a != [rarefy_depth(10, 2, r) for r in range(2000)]


def test_levels_are_nested():
    d = ref.depths(42, 1, 4000)
    prev = np.ones(len(d), dtype=bool)
    for level in range(0, 12):
        keep = d >= level
        assert not (keep & ~prev).any()                                      # a read of level l is a read of every level below
        if level == 0:
            assert keep.all()
        elif level <= 6:
            assert keep.sum() == pytest.approx(len(d) * 2.0 ** -level, rel=0.35)
        prev = keep
