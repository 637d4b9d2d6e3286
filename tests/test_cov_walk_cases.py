"""The corpus of crafted walks (tests/cov_walk_cases.py) on the CPU: every class holds what the GPU cases (tests/test_gpu_cov_walk_edges.py) count on, and
the two independent CPU readings of the reference -- the flat-array C oracle and the literal Python restatement (oracle/ref_literal.py) -- agree on it
bit for bit: bases, covered bases and unique-trio bases by key, and the number of reads the reference would panic on."""
import importlib.util
import os

import numpy as np
import pytest

from tests import cov_walk_cases as cw
from tests.conftest import ROOT
from tests.helpers import oracle_coverage

PCL_WORDS = 2304          # popcount_long_kernel: words of a 64-node stretch its LDS prefix holds (stage_cov.hip)
COV_ITEM_GROUPS = 128     # groups of 64 steps per work item of the short-read kernel (cov_device.hpp)


@pytest.fixture(scope="module")
def corpus():
    from oracle import oracle as orc
    species, rd, classes = cw.build()
    sp = orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in species], [g.range_end for g in species])
    return species, rd, classes, cw.named(), sp, oracle_coverage(species, rd, sp)


def _walks(rd, idx):
    so = rd.step_off.astype(np.int64)
    return [rd.node_id[so[i]:so[i + 1]].astype(np.int64) for i in idx]


def _lens_by_id(species):
    lens = np.zeros(species[-1].range_end + 2, dtype=np.int64)
    for g in species:
        lens[g.range_start:g.range_end + 1] = g.node_len
    return lens


def test_sizes_and_borders(corpus):
    species, rd, classes, info, sp, ref = corpus
    A, B, C = species
    assert A.range_start % 2 == 1 and B.range_start == A.range_end + 1 and C.range_start == B.range_end + 1
    assert 5500 <= A.n_nodes <= 6500 and 2700 <= B.n_nodes <= 3300 and 2200 <= C.n_nodes <= 2800
    assert A.node_len.max() <= 40 and C.node_len.max() <= 40 and A.node_len.min() >= 1
    for lo, hi in ((A, B), (B, C)):                                # a species border INSIDE a block of 2048 ids
        assert lo.range_end // cw.BLOCK == hi.range_start // cw.BLOCK and hi.range_start % cw.BLOCK != 0
    assert B.node_len[cw.GIANT_300K] == 300000 >= 1 << 18 and B.node_len[cw.GIANT_70K] == 70000 > 65536
    assert ((B.node_len >= 65) & (B.node_len <= 1024)).sum() >= 12
    k = np.diff(rd.step_off.astype(np.int64))
    assert int(k.sum()) < 150000
    longer = np.nonzero(k > 64)[0]
    assert np.array_equal(longer, classes["control_long"]) and len(longer) == 3 and (k[longer] == 65).all()
    assert sorted(np.concatenate(list(classes.values())).tolist()) == list(range(rd.n_reads))     # every read is of exactly one class
    # file order is a permutation: the classes are interleaved
    assert np.diff(classes["crowd"]).max() > 1 and classes["fill"].min() < 50
    L, V = sum(int(g.node_len.sum()) for g in species), sum(g.n_nodes for g in species)
    assert L // V >= 48                                            # long_node_shape: the default count of covered bases is popcount_long_kernel


def test_len_edges(corpus):
    species, rd, classes, info, sp, ref = corpus
    lens = _lens_by_id(species)
    seen = set()
    for i, w in zip(classes["len_edges"], _walks(rd, classes["len_edges"])):
        assert sp[i] >= 0 and len(set(np.diff(w).tolist())) <= 1
        where = "first" if w[0] % cw.BLOCK == 0 else "last" if w[0] % cw.BLOCK == cw.BLOCK - 1 else "mid"
        seen.add((int(sp[i]), where, len(w), "up" if len(w) < 2 or w[1] > w[0] else "down"))
        assert 0 <= rd.pstart[i] < lens[w[0]] and rd.pend[i] == lens[w].sum()        # exact: pend - pstart = the walk's bases from pstart
    for s in range(3):
        for where in ("first", "last", "mid"):
            for k in (1, 2, 3, 31, 32, 33, 63, 64):
                assert (s, where, k, "up") in seen and (k == 1 or (s, where, k, "down") in seen)


def test_revisit(corpus):
    species, rd, classes, info, sp, ref = corpus
    ws = _walks(rd, classes["revisit"])
    ps = rd.pstart[classes["revisit"]]
    assert (sp[classes["revisit"]] >= 0).all()
    back0 = {len(w) - 1 for w in ws if len(w) > 2 and w[-1] == w[0] and len(set(w[:-1].tolist())) == len(w) - 1}
    assert {2, 3, 32, 62, 63} <= back0                             # the last step is step 0 again: distances up to STEP_DIST = 63
    assert any(len(w) == 64 and w[-1] == w[1] and w[-1] != w[0] for w in ws)
    assert any(len(w) == 2 and w[0] == w[1] for w in ws) and any(len(w) == 3 and len(set(w.tolist())) == 1 for w in ws)
    assert any(len(w) == 64 and len(set(w.tolist())) == 2 and w[0] != w[1] and (w[::2] == w[0]).all() for w in ws)
    thrice = [w for w in ws if max(np.unique(w, return_counts=True)[1]) == 3 and (w == w[0]).sum() == 1]
    assert thrice and any(w[-1] == w[1] for w in thrice) and any(w[-1] != w[1] for w in thrice)      # first occurrence at step 1, not 0; also as the last step
    assert sum(1 for w, p in zip(ws, ps) if p > 0 and w[-1] == w[0] and len(w) > 2) >= 5             # len0 - pstart is not the node's length


def test_offsets(corpus):
    species, rd, classes, info, sp, ref = corpus
    lens = _lens_by_id(species)
    idx = classes["offsets"]
    ws, ps, pe = _walks(rd, idx), rd.pstart[idx], rd.pend[idx]
    multi = [(w, a, b) for w, a, b in zip(ws, ps, pe) if len(w) > 1]
    one = [(w, a, b) for w, a, b in zip(ws, ps, pe) if len(w) == 1]
    assert len(set(sp[idx].tolist())) == 3 and (sp[idx] >= 0).all()
    seen_of = lambda w, a: int(lens[w[:-1]].sum()) - a
    assert any(a == lens[w[0]] for w, a, b in multi) and all(a <= lens[w[0]] for w, a, b in multi)
    assert any(b < a for w, a, b in multi)
    assert any(0 < b - a < seen_of(w, a) for w, a, b in multi) and any(b - a == seen_of(w, a) for w, a, b in multi)
    assert any(b - a == seen_of(w, a) + 1 for w, a, b in multi) and any(b - a > lens[w].sum() for w, a, b in multi)
    assert any(a < b < lens[w[0]] for w, a, b in one) and any(a == b for w, a, b in one) and any(b < a for w, a, b in one)
    assert any(a == 0 and b == lens[w[0]] for w, a, b in one) and any(b == lens[w[0]] + 1 for w, a, b in one)
    ab = classes["offsets_abort"]
    for i, w in zip(ab, _walks(rd, ab)):
        assert len(w) > 1 and rd.pstart[i] == lens[w[0]] + 1 and sp[i] >= 0           # the assert of profile.rs:854
    assert len(ab) >= 6 and {len(w) for w in _walks(rd, ab)} == {2, 5}


def test_two18_and_giants(corpus):
    species, rd, classes, info, sp, ref = corpus
    lens = _lens_by_id(species)
    idx = classes["two18"]
    ws, span = _walks(rd, idx), rd.pend[idx] - rd.pstart[idx]
    on20 = sorted(int(s) for w, s in zip(ws, span) if len(w) == 1 and w[0] == info["n20"])
    assert lens[info["n20"]] == 20 and on20 == [(1 << 18) - 1] * 2 + [1 << 18] * 2 + [400000] * 2
    n_big = sum(1 for w, s in zip(ws, span) if len(w) == 1 and s >= 1 << 18)
    print("one-node reads of 2^18 bases and more: %d" % n_big)
    assert n_big >= 6                                              # 4 on the 20-base node, 3 on the 300 000-base node (one of them partly)
    g = [(int(rd.pstart[i]), int(rd.pend[i])) for i, w in zip(idx, ws) if len(w) == 1 and w[0] == info["g300"]]
    assert sorted(g) == [(0, 300000), (0, 300001), (5, 299999)]
    assert any(len(w) == 3 and w[1] == info["g300"] for w in ws) and any(len(w) == 2 and w[0] == info["g300"] for w in ws)
    g70 = [w for w in _walks(rd, classes["giant"])]
    assert all(info["g70"] in w for w in g70) and any(len(w) == 1 for w in g70) and any(len(w) > 1 and w[-1] == info["g70"] for w in g70)
    assert (sp[idx] == 1).sum() == 5 and (sp[classes["giant"]] == 1).all()


def test_word_edges_and_stretches(corpus):
    species, rd, classes, info, sp, ref = corpus
    node_len = np.concatenate([g.node_len for g in species])
    bit_off = np.concatenate([[0], np.cumsum(node_len)])
    words = lambda v: int((bit_off[v + 1] - 1) // 32 - bit_off[v] // 32 + 1)
    covered = set(int(w[0]) for w in _walks(rd, classes["words"]) if len(w) == 1)
    for first_id, g0 in zip(info["word_nodes"], info["word_v"]):
        v = lambda j: g0 + j
        assert bit_off[v(0)] % 32 == 0 and tuple(node_len[v(0):v(12)]) == cw.WORD_LENS
        assert node_len[v(1)] == 1 and bit_off[v(1)] % 32 == 31                       # one base on bit 31
        assert node_len[v(2)] == 1 and bit_off[v(2)] % 32 == 0                        # ... on bit 32: bit 0 of the next word
        assert bit_off[v(3) + 1] % 32 == 0 and bit_off[v(3)] % 32 == 1                # ends on bit 31
        assert bit_off[v(4)] % 32 == 0 and words(v(4)) == 1 and node_len[v(4)] == 32  # one whole word
        assert bit_off[v(5)] % 32 == 0 and words(v(5)) == 2 and bit_off[v(6) + 1] % 32 == 0 and words(v(7)) == 2
        assert words(v(11)) == 3 and bit_off[v(11)] % 32 == 30
        assert ((first_id + 1) in covered) != ((first_id + 2) in covered)             # of the two one-base nodes one is covered, its neighbour is not
        assert all(first_id + j in covered for j in (0, 3, 4, 5, 6, 7, 8, 9, 10, 11))
    # the stretches of 64 nodes popcount_long_kernel takes: cooperative (a node over 64 bases, at most PCL_WORDS words) or by the per-lane loop
    V = len(node_len)
    kinds = {}
    for st in range((V + 63) // 64):
        lo, hi = st * 64, min(V, st * 64 + 64)
        wa = (bit_off[lo] // 32) & ~3
        nw = (bit_off[hi] - 1) // 32 - wa + 1
        kinds[st] = ("coop" if nw <= PCL_WORDS and node_len[lo:hi].max() > 64 else "over" if nw > PCL_WORDS else "short", int(nw))
    nA = species[0].n_nodes
    assert kinds[info["word_v"][1] // 64][0] == kinds[(info["word_v"][1] + 11) // 64][0] == "coop"      # B's word-edge nodes
    assert kinds[0][0] == "short"                                                     # A's: the per-lane loop
    k70, k300 = kinds[(nA + cw.GIANT_70K) // 64], kinds[(nA + cw.GIANT_300K) // 64]
    assert k70[0] == "coop" and PCL_WORDS - 128 <= k70[1] <= PCL_WORDS                # just below PCL_WORDS
    assert k300[0] == "over"                                                          # above it
    assert sum(1 for st in kinds if kinds[st][0] == "short" and st * 64 >= nA and st * 64 + 64 <= nA + species[1].n_nodes) >= 2    # no node over 64 bases
    assert all(kinds[(nA + int(m) - species[1].range_start) // 64][0] == "coop" for m in info["mids"])
    # no read of another class steps on a word-edge node, so what is covered there is what the class marks: whole by a flag and also by bits, whole
    # only as the union of two partial marks, all but one base of a whole word, and of the two one-base nodes one
    named = np.concatenate([f + np.arange(12) for f in info["word_nodes"]])
    so = rd.step_off.astype(np.int64)
    owner = np.repeat(np.arange(rd.n_reads), np.diff(so))
    assert set(owner[np.isin(rd.node_id, named)].tolist()) <= set(classes["words"].tolist())
    for first_id, s in zip(info["word_nodes"], (0, 1)):
        lo = first_id - species[s].range_start
        want = list(cw.WORD_LENS)
        want[4] = 31
        want[2 if s else 1] = 0
        assert ref[s][2][lo:lo + 12].tolist() == want, s


def test_far_border_crowd(corpus):
    species, rd, classes, info, sp, ref = corpus
    A, B, C = species
    n_far4096 = 0
    for i, w in zip(classes["far"], _walks(rd, classes["far"])):
        b0 = (w[0] // cw.BLOCK) * cw.BLOCK
        assert sp[i] >= 0 and ((w >= b0 + 2048 + 52) | (w <= b0 - 200)).any()        # outside a window of 2048 nodes from 64 .. 127 in front of the block
        n_far4096 += bool((w >= b0 + 4096).any() and sp[i] == 0)
        assert (w <= b0 - 200).any() or (w >= b0 + 2100).any()
    assert n_far4096 >= 10 and any((w <= (w[0] // cw.BLOCK) * cw.BLOCK - 200).any() and w[-1] // cw.BLOCK == w[0] // cw.BLOCK for w in _walks(rd, classes["far"]))
    far_b = [w for i, w in zip(classes["far"], _walks(rd, classes["far"])) if sp[i] == 1]       # B: from block 4 back into block 3, the giants among the nodes
    assert len(far_b) >= 8 and all(w[0] // cw.BLOCK == 4 and (w // cw.BLOCK == 3).any() for w in far_b)
    assert any(info["g300"] in w[1:-1] for w in far_b) and any(w[-1] == info["g70"] for w in far_b)
    firsts = np.array([w[0] for w in _walks(rd, classes["border"])])
    spb = sp[classes["border"]]
    for lo_s, (lo, hi) in enumerate(((A, B), (B, C))):
        blk = lo.range_end // cw.BLOCK
        assert ((firsts // cw.BLOCK == blk) & (spb == lo_s)).sum() >= 10 and ((firsts // cw.BLOCK == blk) & (spb == lo_s + 1)).sum() >= 10
        assert (firsts == lo.range_end).any() and (firsts == hi.range_start).any()
    assert (spb >= 0).all()
    # crowd: every read starts in the crowd's block, which alone holds more groups of 64 steps than a work item
    so = rd.step_off.astype(np.int64)
    k = np.diff(so)
    first = np.full(rd.n_reads, -1, dtype=np.int64)
    first[k > 0] = rd.node_id[so[:-1][k > 0]]
    in_block = np.nonzero(first // cw.BLOCK == cw.CROWD_BLOCK)[0]
    assert np.array_equal(in_block, classes["crowd"]) and len(in_block) >= 650
    assert 10 <= k[in_block].min() and k[in_block].max() <= 20
    groups = int(k[in_block].sum()) // 64                          # (a lower bound: the layout pads a group rather than cut a walk)
    print("steps of the crowd's block: %d = %d groups and more" % (int(k[in_block].sum()), groups))
    assert groups >= COV_ITEM_GROUPS + 2                           # more than one item at the default cov_item_groups ...
    # ... and not more than two: a group of the block is left with fewer than 64 - 19 steps only where a layout unit ends (build_step_read: units of
    # 2^g buckets of 32 ids, about 2048 steps each)
    T, NB, g = int(k.sum()), (int(rd.node_id.max()) >> 5) + 1, 0
    while g < 12 and T / NB * (1 << g) < 2048.0:
        g += 1
    units = max(cw.BLOCK >> (5 + g), 1)
    assert int(k[in_block].sum()) // (64 - 19) + units + 1 <= 2 * COV_ITEM_GROUPS
    assert (k[classes["fill"]] >= 1).all() and (k[classes["fill"]] <= 64).all() and len(classes["fill"]) >= 1900
    assert {1, 2, 3, 63, 64} <= set(k[classes["fill"]].tolist())
    assert (k[classes["empty"]] == 0).all() and len(classes["empty"]) >= 3
    assert (sp[classes["control_u"]] == -1).all() and len(classes["control_u"]) == 2 and (sp[classes["fill"]] >= 0).all()


def test_heads(corpus):
    """a middle node with four and more unique rows; reads that search EVERY row of such a head, from either side, so whatever the order the
    rows are filed in, rows at index 2 and beyond are found (the j >= 2 loop of the lookup) -- by walks of 64 steps, whose step i is lane i of a
    group: the hub windows end on lanes 2 (3) and 63 (62)"""
    species, rd, classes, info, sp, ref = corpus
    C = species[2]
    T, bases, cov, tb, na = ref[2]
    assert C.n_paths >= 6
    for m in cw.HUBS:
        rows = np.nonzero(T.abc[:, 1] == m)[0]
        assert len(rows) == cw.N_DIV >= 4 and len(set(T.hap[rows].tolist())) == cw.N_DIV          # one row per diverging path
        assert (tb[rows] > 0).all()                                                                  # every row of the head is hit
    assert (C.range_start + cw.HUBS[-1]) % cw.BLOCK == cw.BLOCK - 1
    xyx = np.nonzero((T.abc[:, 0] == T.abc[:, 2]))[0]
    assert len(xyx) == 2 and (tb[xyx] > 0).all()                                                     # a == c
    rev = np.nonzero((T.hap == cw.N_DIV) & (T.abc[:, 1] >= cw.REV))[0]
    assert len(rev) >= 2 and (tb[rev] > 0).all()                                                     # rows of the path that runs down
    k = np.diff(rd.step_off.astype(np.int64))
    assert (k[classes["heads64"]] == 64).all() and (sp[classes["heads64"]] == 2).all() and (sp[classes["heads"]] == 2).all()
    lanes = set()
    for w in _walks(rd, classes["heads64"]):
        lanes |= {i for i in range(2, 64) if w[i - 1] - C.range_start in cw.HUBS}
    assert lanes == {2, 3, 62, 63}
    mids = {int(w[1]) - C.range_start for w in _walks(rd, classes["heads"]) if len(w) == 3}
    ups = [w for w in _walks(rd, classes["heads"]) if len(w) == 3]
    assert set(cw.HUBS) <= mids and any(w[0] < w[2] for w in ups) and any(w[0] > w[2] for w in ups)


def _literal():
    # by file path: oracle/oracle.py shadows the package `oracle` once its directory is on sys.path
    spec = importlib.util.spec_from_file_location("cov_walk_ref_literal", os.path.join(ROOT, "oracle", "ref_literal.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_c_oracle_equals_literal_restatement(corpus):
    species, rd, classes, info, sp, ref = corpus
    lit = _literal()
    so = rd.step_off.astype(np.int64)
    aborts = 0
    for si, g in enumerate(species):
        T, bases, cov, tb, na = ref[si]
        nodes_len = [int(x) for x in g.node_len]
        paths = {g.hap_names[h]: [int(x) for x in g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])]] for h in range(g.n_paths)}
        uniq, ulen, rows = lit.trio_nodes_info(nodes_len, paths)
        reads = [dict(path="".join(">%d" % v for v in rd.node_id[so[i]:so[i + 1]]), read_start=int(rd.pstart[i]), read_end=int(rd.pend[i]))
                 for i in np.nonzero(sp == si)[0]]
        _, _, l_cov, l_bases, l_tb, l_abort = lit.get_node_abundances(nodes_len, uniq, ulen, g.range_start - 1, reads)
        assert [int(x) for x in bases] == l_bases and [int(x) for x in cov] == l_cov
        got = {tuple(int(x) for x in T.abc[i]): (int(T.len[i]), int(tb[i])) for i in range(T.n_unique)}
        assert got == {key: (ulen[i], l_tb[i]) for key, i in uniq.items()}
        assert na == l_abort
        assert int(bases.sum()) > 0 and int(tb.sum()) > 0
        aborts += na
    n_assert = sum(1 for i in classes["offsets_abort"] if sp[i] >= 0 and so[i + 1] - so[i] > 1)
    assert aborts == n_assert > 0


def test_shifted_ids_widen_the_buckets(corpus):
    """the corpus 32 768 ids higher (the group_bucket_bits case of the GPU file): more than 2^10 buckets of 32 ids, so build_step_read's `++shift` runs under
    the option's least cap and not under the default one; blocks, borders and the reference's results stay as they are"""
    from oracle import oracle as orc
    species, rd, classes, info, sp, ref = corpus
    sp_s, rd_s = cw.shifted(species, rd)
    assert ((int(rd.node_id.max()) >> 5) + 1 <= 1 << 10) and ((int(rd_s.node_id.max()) >> 5) + 1 > 1 << 10)      # unshifted: the option changes nothing
    assert (int(rd_s.node_id.max()) >> 5) + 1 <= 1 << 24 and (int(rd_s.node_id.max()) >> 6) + 1 <= 1 << 10        # default cap: 32-id buckets; cap 2^10: 64-id buckets
    assert cw.ID_SHIFT % cw.BLOCK == 0 and np.array_equal(rd_s.node_id % cw.BLOCK, rd.node_id % cw.BLOCK)
    assert np.array_equal(rd_s.step_off, rd.step_off) and np.array_equal(rd_s.pstart, rd.pstart) and np.array_equal(rd_s.pend, rd.pend)
    assert np.array_equal(orc.bin_reads(rd_s.step_off, rd_s.node_id, [g.range_start for g in sp_s], [g.range_end for g in sp_s]), sp)
    for (T, b, c, t, na), (T2, b2, c2, t2, na2) in zip(ref, oracle_coverage(sp_s, rd_s, sp)):
        assert np.array_equal(b, b2) and np.array_equal(c, c2) and np.array_equal(t, t2) and na == na2 and np.array_equal(T.abc, T2.abc)
