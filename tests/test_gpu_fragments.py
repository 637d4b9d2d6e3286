"""GPU tests of the fragment support (pantax_hip_fragment_mates, pantax_hip_strain_fragments, --strain-fragments).  The expected integers come from the
row-by-row reading of the contract in tests/fragments_ref.py (pinned by hand in tests/test_fragments_ref.py); everything compares element for element."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import fragments_ref as ref
from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile

pytestmark = pytest.mark.gpu

E_INVALID, E_LIMIT, E_STATE = -1, -4, -7
NONE, AMB = ref.MATE_NONE, ref.MATE_AMBIGUOUS
TAG_PAIRS = [(a, b) for a in range(3) for b in range(3)]


@pytest.fixture(scope="module")
def engine():
    from pantax_amd.engine import Engine
    with Engine(0) as eng:
        yield eng


# ---- mates ---------------------------------------------------------------------------------------------------------------------

def _crafted(n, seed):
    """n reads whose keys are small integers, so that the sorted order is the key order: runs of 1 .. 4 equal keys; a valid pair sits at the sorted
    positions 63/64 and 255/256 (two waves, two workgroups) and at the end of the array, the last one being the first and the last READ; the pairs
    cycle through all nine tag pairs.  -> (key [n], tag [n]) in read order"""
    rng = np.random.default_rng(seed)
    forced = {p: t for p, t in ((63, (0, 0)), (255, (2, 1)), (n - 2, (1, 2))) if 0 <= p and p + 2 <= n}
    starts = sorted(forced)
    run_of, tag_at, pos, run, cycle = [], [], 0, 0, 0
    while pos < n:
        if pos in forced:
            L, tags = 2, list(forced[pos])
        else:
            room = min([s for s in starts if s > pos] + [n]) - pos
            L = int(min(rng.integers(1, 5), room))
            if L == 2:
                tags = list(TAG_PAIRS[cycle % 9])
                cycle += 1
            else:
                tags = rng.integers(0, 3, size=L).tolist()
        run += 1
        run_of += [run] * L
        tag_at += tags
        pos += L
    perm = rng.permutation(n)                                                  # sorted position -> read
    if n >= 2:                                                                 # the last pair: reads 0 and n - 1
        for want, p in ((0, n - 2), (n - 1, n - 1)):
            q = int(np.nonzero(perm == want)[0][0])
            perm[q], perm[p] = perm[p], perm[q]
    key, tag = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    key[perm] = np.array(run_of, dtype=np.uint64)
    tag[perm] = np.array(tag_at, dtype=np.uint8)
    return key, tag


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 5003])
def test_mates_equal_reference(engine, n):
    key, tag = _crafted(n, 100 + n)
    exp_mate, exp_counts = ref.fragment_mates(key, tag)
    if n >= 2:
        assert exp_mate[0] == n - 1 and exp_mate[n - 1] == 0                   # the mates that are the first and the last read
    if n >= 257:
        assert exp_counts[0] >= 3 and exp_counts[1] > 0 and exp_counts[2] > 0 and exp_counts[3] > 0
        runs = {}
        for i, k in enumerate(key.tolist()):
            runs.setdefault(k, []).append(int(tag[i]))
        assert {tuple(sorted(t)) for t in runs.values() if len(t) == 2} == {tuple(sorted(t)) for t in TAG_PAIRS} and {len(t) for t in runs.values()} == {1, 2, 3, 4}
    for _ in range(2):                                                         # twice: the same bits
        mate, counts = engine.fragment_mates(key, tag)
        assert mate.dtype == np.uint32 and np.array_equal(mate, exp_mate)
        assert counts.dtype == np.uint64 and np.array_equal(counts, exp_counts)


def test_mates_from_ids(engine):
    """64-bit keys (eight sort passes) from real ids through the binding: X/1 with X/2, an id twice, singles, a triple, X/1 twice, X/1 beside the bare X"""
    from pantax_amd.engine import fragment_key
    ids = []
    for i in range(700):
        ids += [b"S0R%d/1" % i, b"S0R%d/2" % i]
    ids += [b"dup%d" % (i // 2) for i in range(300)] + [b"one%d" % i for i in range(200)] + [b"t"] * 3 + [b"q/1", b"q/1", b"w/1", b"w", b"v/2", b"a/1", b"a/", b"/1", b"x/3"]
    rng = np.random.default_rng(5)
    ids = [ids[i] for i in rng.permutation(len(ids))]
    kt = [fragment_key(i) for i in ids]
    assert kt == [ref.fragment_key(i) for i in ids]
    key, tag = np.array([k for k, _ in kt], dtype=np.uint64), np.array([t for _, t in kt], dtype=np.uint8)
    exp_mate, exp_counts = ref.fragment_mates(key, tag)
    assert exp_counts.tolist() == [850, 200 + 5, 3 + 2 + 2, 1]
    mate, counts = engine.fragment_mates(key, tag)
    assert np.array_equal(mate, exp_mate) and np.array_equal(counts, exp_counts)


def test_mates_arguments(engine):
    from pantax_amd.engine import p
    key, tag = np.array([4, 4, 9], dtype=np.uint64), np.array([1, 3, 0], dtype=np.uint8)
    mate, counts = np.full(3, 77, dtype=np.uint32), np.full(4, 77, dtype=np.uint64)
    lib = engine.lib
    assert lib.pantax_hip_fragment_mates(engine.ctx, 3, p(key), p(tag), p(mate), p(counts)) == E_INVALID           # a tag above 2
    assert lib.pantax_hip_fragment_mates(engine.ctx, 0xFFFFFFFE, p(key), p(tag), p(mate), p(counts)) == E_LIMIT    # (refused before anything is read)
    tag[1] = 2
    assert lib.pantax_hip_fragment_mates(engine.ctx, 3, None, p(tag), p(mate), p(counts)) == E_INVALID
    assert lib.pantax_hip_fragment_mates(engine.ctx, 3, p(key), p(tag), p(mate), None) == E_INVALID
    assert np.all(mate == 77) and np.all(counts == 77)
    assert lib.pantax_hip_fragment_mates(engine.ctx, 3, p(key), p(tag), p(mate), p(counts)) == 0
    assert mate.tolist() == [1, 0, NONE] and counts.tolist() == [1, 1, 0, 0]


# ---- the fragment pass -----------------------------------------------------------------------------------------------------------

def _members(g, haps):
    """per species-local node the positions of `haps` whose walk visits it"""
    out = [set() for _ in range(g.n_nodes)]
    for p, h in enumerate(haps):
        for v in set(g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])].tolist()):
            out[v].add(p)
    return out


def _build():
    """Ten species as in the read rescue test: four tiny ones (their reads share one 64-step group with their neighbours'; K_s = 1 and 2), K_s = 0, a
    4-haplotype species with all four as candidates (the hand-placed fragments; two of its weights tie), a 64-haplotype species with K_s = 64 (bit 63), a
    70-haplotype species with K_s = 70 (skipped), one of K_s = 1 and one that is left out of the db.  Short reads of the generator, mated at random
    within their species, plus hand-placed walks composed node by node from the membership of every node."""
    import synthdata as synth
    from oracle import oracle as orc
    rng = np.random.default_rng(8)
    shapes = [(2, 250), (3, 250), (2, 250), (3, 250), (1, 8000), (4, 8000), (64, 8000), (70, 8000), (3, 6000), (3, 6000)]
    species, start = [], 1
    for i, (H, glen) in enumerate(shapes):
        g = synth.make_species(rng, str(1000 + i), H, glen, start, "GCF_%06d" % (i + 1), present_frac=0.6)
        species.append(g)
        start = g.range_end + 1
    rd = synth.make_reads(rng, species[4:], 2500, adversarial_frac=0.0)
    picks = [[0], [1, 0], [0], [2, 0], [], [3, 1, 0, 2], list(range(63, -1, -1)), rng.permutation(70).tolist(), [1]]
    weights = [[1.0], [2.0, 2.0], [3.0], [0.5, 4.0], [], [2.5, 2.5, 1.0, 0.25], rng.choice([1.0, 2.5, 7.25], size=64).tolist(), (rng.random(70) * 10 + 0.1).tolist(), [1.0]]
    M = [_members(g, x) for g, x in zip(species, picks)]
    walks, ps, pe, marks = [], [], [], {}

    def add(s, local_nodes, name, pstart=3, pend=40):
        marks.setdefault(name, []).append(len(walks))
        walks.append(np.asarray(local_nodes, dtype=np.uint32) + np.uint32(species[s].range_start) if s is not None else np.zeros(0, dtype=np.uint32))
        ps.append(pstart)
        pe.append(pend)

    def pool(s, pred):
        out = [v for v in range(species[s].n_nodes) if pred(M[s][v])]
        assert out, "no such node in species %d" % s
        return out

    def fill(nodes, n):
        return [nodes[i % len(nodes)] for i in range(n)]

    # species 5, positions in the list [3, 1, 0, 2]: 0 = haplotype 3, 1 = haplotype 1, 2 = haplotype 0, 3 = haplotype 2.  A walk over x_only + y_only
    # fits nobody; a walk inside `core` fits everybody
    core = pool(5, lambda m: m == {0, 1, 2, 3})
    only = [pool(5, lambda m, p=p: m == {p}) for p in range(4)]
    two = {pq: pool(5, lambda m, pq=pq: m == set(pq)) for pq in ((0, 3), (1, 2))}     # the two clades
    near = sorted(core)[:4]
    far = sorted(core)[-2:]
    add(5, near[:2], "same_group"); add(5, near[2:4], "same_group")                   # neighbours in slot order
    add(5, near[:1], "other_group"); add(5, far, "other_group")                       # the two ends of the species
    add(5, core[:2], "other_species"); add(6, list(range(3)), "other_species")
    add(5, core[:2], "mate_dropped"); add(5, core[2:4], "mate_dropped")
    add(5, core[:2], "mate_no_walk"); add(None, [], "mate_no_walk")
    add(5, core[:2], "mate_outside_db"); add(9, list(range(3)), "mate_outside_db")
    add(5, fill(two[(0, 3)], 64), "long64"); add(5, only[0][:1], "long64")            # C = {0, 3} & {0}
    add(5, fill(two[(1, 2)], 65), "long65"); add(5, only[2][:2], "long65")            # more than 64 steps: C = {1, 2} & {2}
    add(5, fill(core, 129) + only[3][:1], "long130"); add(5, fill(two[(0, 3)], 70), "long130")   # both long: {3} & {0, 3}
    add(5, [only[1][0], core[0]], "same_walk"); add(5, [only[1][0], core[0]], "same_walk")
    add(5, core[:3], "concordant"); add(5, two[(0, 3)][:2], "concordant")             # F = {0, 3}: positions 0 and 3 weigh 2.5 and 0.25
    add(5, [two[(0, 3)][0], core[1]], "unique_by_pair"); add(5, [core[0], only[0][0]], "unique_by_pair_not")   # {0, 3} & {0}: F = {0}, but a mate names it alone
    add(5, two[(0, 3)][:1], "unique_by_pair2"); add(5, pool(5, lambda m: m == {0, 1, 2})[:1], "unique_by_pair2")   # {0, 3} & {0, 1, 2}: only the pair names position 0
    add(5, pool(5, lambda m: m == {0, 1, 3})[:1], "tie"); add(5, pool(5, lambda m: m == {0, 1, 2})[:1], "tie")   # F = {0, 1}, equal weights: haplotype 1 (position 1)
    add(5, two[(1, 2)][:1], "discordant"); add(5, only[0][:1], "discordant")          # {1, 2} & {0}: filed at (position 1: the tie goes to haplotype ... , 0)
    add(5, [only[0][0], only[1][0]], "half"); add(5, core[:1], "half")                # {} & everybody
    add(5, [only[0][0], only[1][0]], "unexplained"); add(5, [only[2][0], only[3][0]], "unexplained")
    for s in (0, 1, 2, 3, 0, 1, 2, 3):                                                # the four tiny species: one group, mated within their species
        add(s, list(range(min(3, species[s].n_nodes))), "tiny")
    add(4, list(range(4)), "k0"); add(4, list(range(2, 6)), "k0")
    add(6, pool(6, lambda m: 63 in m and 0 in m)[:5], "wide64"); add(6, pool(6, lambda m: 0 in m)[:5], "wide64")
    add(7, list(range(5)), "skipped"); add(7, list(range(3, 9)), "skipped")
    add(8, list(range(3)), "triple"); add(8, list(range(3)), "triple"); add(8, list(range(3)), "triple")
    k = np.array([len(x) for x in walks], dtype=np.uint64)
    n = len(walks)
    one = lambda v: np.full(n, v, dtype=np.int64)
    reads = synth.PackedReads(np.concatenate([rd.step_off, rd.step_off[-1] + np.cumsum(k)]), np.concatenate([rd.node_id] + walks), None,
                              np.concatenate([rd.pstart, np.array(ps, dtype=np.int64)]), np.concatenate([rd.pend, np.array(pe, dtype=np.int64)]),
                              np.concatenate([rd.qlen, one(30000)]), np.concatenate([rd.mapq, one(60)]), np.concatenate([rd.plen, one(30000)]))
    R = reads.n_reads
    hand0 = R - n
    flags = np.zeros(R, dtype=np.uint8)
    flags[rng.choice(hand0, size=60, replace=False)] = rng.choice([1, 2], size=60).astype(np.uint8)
    flags[hand0 + marks["mate_dropped"][1]] = 1
    db = species[:9]                                                           # the last species is not in the db
    # mates: the hand-placed walks in pairs as they were added (the tiny ones within their species, the triple ambiguous); the generator's reads of
    # every species shuffled and mated two by two, but for some singles, some ambiguous ones and a few mated across species
    mate = np.full(R, NONE, dtype=np.uint32)
    hand_at = {name: [hand0 + i for i in idx] for name, idx in marks.items()}
    for name, idx in hand_at.items():
        if name == "tiny":
            for a, b in zip(idx[:4], idx[4:]):
                mate[a], mate[b] = b, a
        elif name == "triple":
            mate[idx] = AMB
        elif name == "unique_by_pair":
            a, b = idx[0], hand_at["unique_by_pair_not"][0]
            mate[a], mate[b] = b, a
        elif name != "unique_by_pair_not":
            for a, b in zip(idx[0::2], idx[1::2]):
                mate[a], mate[b] = b, a
    sp_all = orc.bin_reads(reads.step_off, reads.node_id, [g.range_start for g in species], [g.range_end for g in species])
    left = []
    for s in range(4, 10):
        idx = rng.permutation(np.nonzero(sp_all[:hand0] == s)[0])
        cut = len(idx) * 8 // 10 // 2 * 2
        for a, b in zip(idx[0:cut:2], idx[1:cut:2]):
            mate[a], mate[b] = b, a
        rest = idx[cut:]
        mate[rest[:len(rest) // 3]] = AMB
        left += rest[len(rest) // 3:2 * len(rest) // 3].tolist()                # ... the last third stays single
    left = rng.permutation(left)
    for a, b in zip(left[0::2], left[1::2]):                                    # across species, now and then within one
        mate[a], mate[b] = b, a
    picks_off = np.cumsum([0] + [len(x) for x in picks]).astype(np.uint64)
    cands = (picks_off, np.array(sum(picks, []), dtype=np.uint32), np.array(sum(weights, []), dtype=np.float64))
    return db, reads, flags, cands, mate, M, hand_at


def _rows(db, reads, flags):
    from oracle import oracle as orc
    sp = orc.bin_reads(reads.step_off, reads.node_id, [g.range_start for g in db], [g.range_end for g in db])
    so = reads.step_off.astype(np.int64)
    rows = []
    for r in range(reads.n_reads):
        s = int(sp[r]) if so[r + 1] > so[r] else -1
        nodes = (reads.node_id[so[r]:so[r + 1]].astype(np.int64) - db[s].range_start).tolist() if s >= 0 else []
        rows.append((s, flags[r] == 0, nodes, int(reads.pstart[r]), int(reads.pend[r])))
    return sp, rows


def _hap_nodes(db):
    return [[set(g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])].tolist()) for h in range(g.n_paths)] for g in db]


def _fixture_holds_the_cases(db, reads, flags, cands, mate, M, hand_at, rows, exp):
    """what the hand-placed fragments are meant to be and that no class is empty, from the reference alone: a set that leaves a class empty hides a failure"""
    hap, species, status, pair_off, pair, n = exp
    off, ch, cw = cands
    assert ref.check_mates(mate)
    K = np.diff(off.astype(np.int64))
    assert K.tolist() == [1, 2, 1, 2, 0, 4, 64, 70, 1] and status.tolist() == [0, 0, 0, 0, 1, 0, 0, E_LIMIT, 0] and 63 in ch[int(off[6]):int(off[7])].tolist()
    assert (species[:, :, 0].sum(axis=0) > 0).all() and (species[5, :, 0] > 0).all()                  # every one of the nine classes holds something, species 5 all of them
    assert (hap[:, :, 0].sum(axis=0) > 0).all() and (hap[int(off[5]):int(off[6]), ref.COMPATIBLE, 0] > 0).all() and hap[int(off[6]):int(off[7]), ref.COMPATIBLE, 0].sum() > 0
    assert pair[int(pair_off[5]):int(pair_off[6])].sum() >= 2 and pair_off.tolist() == np.cumsum([0, 1, 4, 1, 4, 0, 16, 4096, 0, 1]).tolist()
    assert not species[4, ref.CONCORDANT:ref.UNEXPLAINED + 1].any() and species[4, ref.PAIRED, 0] >= 1 and species[4, ref.COUNTED, 0] > 10
    assert not species[7, ref.CONCORDANT:ref.UNEXPLAINED + 1].any() and species[7, ref.PAIRED, 0] >= 1 and not hap[int(off[7]):int(off[8])].any()
    assert (species[[0, 1, 2, 3], ref.COUNTED, 0] == 2).all() and (species[[0, 1, 2, 3], ref.PAIRED, 0] == 1).all() and species[8, ref.MULTI, 0] >= 3
    k = np.diff(reads.step_off.astype(np.int64))
    want = {"same_group": 4, "other_group": 4, "long64": 1, "long65": 1, "long130": 1, "same_walk": 1, "concordant": 2, "unique_by_pair": 1, "unique_by_pair2": 1,
            "tie": 2, "discordant": 0, "half": 0, "unexplained": 0, "wide64": None, "mate_dropped": -1, "mate_no_walk": -1, "mate_outside_db": -1, "other_species": -1,
            "k0": -1, "skipped": -1, "triple": -1}
    for name, f in want.items():
        a = hand_at[name][0]
        if f is not None:
            assert n[a] == f, (name, n[a])
        if f is not None and f >= 0:
            assert n[int(mate[a])] == f
    assert n[hand_at["wide64"][0]] >= 1 and n[hand_at["mate_no_walk"][1]] == -2 and n[hand_at["mate_outside_db"][1]] == -2 and n[hand_at["mate_dropped"][1]] == -1
    assert sorted(k[hand_at["long64"]].tolist()) == [1, 64] and sorted(k[hand_at["long65"]].tolist()) == [2, 65] and sorted(k[hand_at["long130"]].tolist()) == [70, 130]
    assert k[hand_at["mate_no_walk"][1]] == 0
    c5 = lambda r: ref._one_read(_fixture_holds_the_cases.hap_nodes, rows[r], off, ch, cw)[0]
    e5 = int(off[5])
    assert [c - e5 for c in c5(hand_at["unique_by_pair2"][0])] == [0, 3] and [c - e5 for c in c5(hand_at["unique_by_pair"][0])] == [0, 3]
    assert [c - e5 for c in c5(hand_at["discordant"][0])] == [1, 2] and [c - e5 for c in c5(hand_at["discordant"][1])] == [0]
    assert c5(hand_at["half"][0]) == [] and len(c5(hand_at["half"][1])) == 4 and c5(hand_at["unexplained"][0]) == [] and c5(hand_at["unexplained"][1]) == []
    t0 = hand_at["tie"][0]
    tie = ref.strain_fragments(_fixture_holds_the_cases.hap_nodes, [rows[t0], rows[t0 + 1]], off, ch, cw, [1, 0])[0]
    assert tie[e5:e5 + 4, ref.ASSIGNED, 0].tolist() == [0, 1, 0, 0] and tie[e5:e5 + 4, ref.COMPATIBLE, 0].tolist() == [1, 1, 0, 0] and cw[e5] == cw[e5 + 1]
    # the discordant fragment is filed at (position 1, position 0): haplotype 1 (weight 2.5) beats haplotype 0 (weight 1.0)
    m5 = pair[int(pair_off[5]):int(pair_off[6])].reshape(4, 4)
    assert m5[1, 0] >= 1 and m5[0, 1] == m5[1, 0]
    assert hap[e5:e5 + 4, ref.UNIQUE_BY_PAIR, 0].sum() >= 1 and hap[e5, ref.UNIQUE, 0] > hap[e5, ref.UNIQUE_BY_PAIR, 0]
    sp = np.array([r[0] for r in rows])
    assert (sp < 0).sum() > 5 and ((sp >= 0) & (flags != 0)).sum() > 10                                # "U" reads, dropped reads
    ref.check_identities(hap, species, status, pair_off, pair, off)


@pytest.fixture(scope="module")
def stage():
    from pantax_amd.engine import Engine
    db, reads, flags, cands, mate, M, hand_at = _build()
    sp, rows = _rows(db, reads, flags)
    hap_nodes = _hap_nodes(db)
    exp = ref.strain_fragments(hap_nodes, rows, *cands, mate)
    _fixture_holds_the_cases.hap_nodes = hap_nodes
    _fixture_holds_the_cases(db, reads, flags, cands, mate, M, hand_at, rows, exp)      # on the CPU, before any GPU run
    eng = Engine(0)
    eng.upload_db(db)
    eng.upload_reads(reads.step_off, reads.node_id, reads.pstart, reads.pend, reads.qlen, reads.mapq, flags)
    eng.rcls_profile(want_species=False)
    yield eng, db, reads, flags, cands, mate, rows, hap_nodes, exp
    eng.close()


def _same(got, exp):
    assert len(got) == len(exp) == 6
    for g, e in zip(got, exp):
        assert g.dtype == e.dtype and g.shape == e.shape
        assert np.array_equal(g, e)


def test_stage_call_equals_reference(stage, set_opt):
    eng, db, reads, flags, cands, mate, rows, hap_nodes, exp = stage
    _same(eng.strain_fragments(*cands, mate, want_n=True), exp)
    _same(eng.strain_fragments(*cands, mate, want_n=True), exp)                       # twice: the same bits
    got = eng.strain_fragments(*cands, mate)                                          # without frag_n_out
    assert got[5] is None
    _same(got[:5] + (exp[5],), exp)
    set_opt(eng, "read_strain_route", "walk")                                         # every species through the compact walk masks
    _same(eng.strain_fragments(*cands, mate, want_n=True), exp)


def test_identities_and_read_support(stage):
    eng, db, reads, flags, cands, mate, rows, hap_nodes, exp = stage
    hap, species, status, pair_off, pair, n = eng.strain_fragments(*cands, mate)
    sup_species = eng.strain_read_support(*cands)[1]
    ref.check_identities(hap, species, status, pair_off, pair, cands[0], sup_species)
    # every mate NONE: single = counted and every other class is zero
    hap0, species0, status0, _, pair0, n0 = eng.strain_fragments(*cands, np.full(len(mate), NONE, dtype=np.uint32), want_n=True)
    assert np.array_equal(species0[:, ref.SINGLE], species0[:, ref.COUNTED]) and np.array_equal(species0[:, ref.COUNTED], sup_species[:, 0])
    assert not species0[:, ref.PAIRED:ref.UNEXPLAINED + 1].any() and not species0[:, ref.MULTI:].any() and not hap0.any() and not pair0.any()
    assert np.array_equal(status0, status) and np.array_equal(n0, np.where(exp[5] == -2, -2, -1))


def _raw(eng, cands, mate, n_species=None, pair_cap=None, fill=77):
    from pantax_amd import _ffi
    from pantax_amd.engine import p
    off, ch, cw = [np.ascontiguousarray(x) for x in cands]
    mt = np.ascontiguousarray(mate, dtype=np.uint32)
    S = eng.S
    cs = _ffi.ReadStrainSet(S if n_species is None else n_species, off.ctypes.data, ch.ctypes.data, cw.ctypes.data)
    k = np.diff(off.astype(np.int64))
    n_pair = int((k[k <= 64] ** 2).sum())
    out = [np.full((max(len(ch), 1), 4, 3), fill, dtype=np.uint64), np.full((S, 9, 3), fill, dtype=np.uint64), np.full(S, fill, dtype=np.int32),
           np.full(S + 1, fill, dtype=np.uint64), np.full(max(n_pair, 1), fill, dtype=np.uint64), np.full(max(len(mt), 1), fill, dtype=np.int32)]
    rc = eng.lib.pantax_hip_strain_fragments(eng.ctx, eng.db, eng.reads, C.byref(cs), p(mt), p(out[0]), p(out[1]), p(out[2]), p(out[3]),
                                             n_pair if pair_cap is None else pair_cap, p(out[4]), p(out[5]))
    return rc, out


def test_cap_protocol_and_arguments(stage):
    eng, db, reads, flags, cands, mate, rows, hap_nodes, exp = stage
    off, ch, cw = cands
    rc, out = _raw(eng, cands, mate)
    assert rc == 0 and all(np.array_equal(o[:len(e)], e) for o, e in zip(out[:5], exp[:5]))
    assert np.array_equal(out[5], np.where(exp[5] == -2, 77, exp[5]))                # reads that are not binned keep what the caller put there
    for cap in (0, int(exp[3][-1]) - 1):                                              # too small: pair_off_out and nothing else
        rc, out = _raw(eng, cands, mate, pair_cap=cap)
        assert rc == E_LIMIT and np.array_equal(out[3], exp[3]) and all(np.all(o == 77) for i, o in enumerate(out) if i != 3)
    R = len(mate)
    pairs = [r for r in range(R) if mate[r] < AMB]
    a = pairs[0]
    b = next(r for r in pairs if r != a and r != mate[a])
    bad = []
    m = mate.copy(); m[a] = b; bad.append(m)                                           # asymmetric: b names another read
    m = mate.copy(); m[a] = a; bad.append(m)                                           # its own mate
    m = mate.copy(); m[a] = R; bad.append(m)                                           # at R ...
    m = mate.copy(); m[a] = 0xFFFFFFFD; bad.append(m)                                  # ... and far above it
    m = mate.copy(); m[int(np.nonzero(mate == NONE)[0][0])] = a; bad.append(m)         # a single that names a mated read
    for m in bad:
        assert not ref.check_mates(m)
        rc, out = _raw(eng, cands, m)
        assert rc == E_INVALID and all(np.all(o == 77) for o in out)                   # before anything is written
    rc, out = _raw(eng, (off[:-1], ch[:int(off[-2])], cw[:int(off[-2])]), mate, n_species=eng.S - 1)
    assert rc == E_INVALID and all(np.all(o == 77) for o in out)
    twice = ch.copy()
    twice[int(off[5]) + 1] = twice[int(off[5])]
    rc, out = _raw(eng, (off, twice, cw), mate)
    assert rc == E_INVALID and all(np.all(o == 77) for o in out)
    rc, out = _raw(eng, cands, mate)                                                   # and the call is whole again
    assert rc == 0 and np.array_equal(out[1], exp[1])


def test_state(stage):
    """reads that are not binned, or binned against another db, are refused as by pantax_hip_strain_read_support; the outputs are left as given"""
    from pantax_amd._ffi import PantaxHipError
    from pantax_amd.engine import Engine
    eng, db, reads, flags, cands, mate, rows, hap_nodes, exp = stage
    with Engine(0) as e2:
        e2.upload_db(db)
        e2.upload_reads(reads.step_off, reads.node_id, reads.pstart, reads.pend, reads.qlen, reads.mapq, flags)
        with pytest.raises(PantaxHipError) as e:
            e2.strain_fragments(*cands, mate)                  # not binned yet
        assert e.value.code == E_STATE
        rc, out = _raw(e2, cands, mate)
        assert rc == E_STATE and all(np.all(o == 77) for o in out)
        e2.rcls_profile(want_species=False)
        e2.upload_db(db)                                       # a new db: the reads were binned against the previous one
        with pytest.raises(PantaxHipError) as e:
            e2.strain_fragments(*cands, mate)
        assert e.value.code == E_STATE


# ---- the file seam -----------------------------------------------------------------------------------------------------------

HEADER = ["species_taxid", "strain_taxid", "genome_ID", "class", "n_fragments", "n_reads", "n_steps", "span", "fraction", "other_strain_taxid", "other_genome_ID"]


def _ids(sset):
    """read ids of the test's own making: within every species the reads in pairs X/1 + X/2, then pairs under one bare id, singles, a triple and an X/1
    twice; a few pairs across the two species (the bare ones among them fall to the duplicate-id rule)"""
    from oracle import oracle as orc
    rd = sset.reads
    rng = np.random.default_rng(3)
    sp = orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in sset.species], [g.range_end for g in sset.species])
    ids = ["solo%d" % r for r in range(rd.n_reads)]
    cross = []
    for s in range(len(sset.species)):
        idx = rng.permutation(np.nonzero(sp == s)[0]).tolist()
        cross += idx[:8]
        idx = idx[8:]
        n = len(idx)
        for j, (a, b) in enumerate(zip(idx[0:n // 2:2], idx[1:n // 2:2])):
            ids[a], ids[b] = "s%dF%d/1" % (s, j), "s%dF%d/2" % (s, j)
        for j, (a, b) in enumerate(zip(idx[n // 2:3 * n // 4:2], idx[n // 2 + 1:3 * n // 4:2])):
            ids[a] = ids[b] = "s%dD%d" % (s, j)
        for a in idx[3 * n // 4:3 * n // 4 + 3]:
            ids[a] = "s%dT" % s
        for a in idx[3 * n // 4 + 3:3 * n // 4 + 5]:
            ids[a] = "s%dQ/1" % s
    for j, (a, b) in enumerate(zip(cross[:8], cross[8:])):                     # one read of either species
        ids[a], ids[b] = ("x%d/2" % j, "x%d/1" % j) if j % 2 else ("xd%d" % j, "xd%d" % j)
    return ids, sp


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import synthdata as synth
    from pantax_amd.engine import Engine
    sset = synth.make_set(41, 2, 5, 6000, 30000, present_frac=0.6, with_ids=True)
    ids, sp = _ids(sset)
    sset.reads.read_id[:] = ids
    root = tmp_path_factory.mktemp("pantax_fragments")
    db = root / "db"
    db.mkdir()
    synth.write_db(sset, str(db))
    gaf = root / "gfa_mapped.gaf"
    synth.write_gaf(sset.reads, str(gaf))
    with Engine(0) as e:
        yield sset, root, db, gaf, e, ids, sp


def _same_rows(got, exp):
    assert len(got) == len(exp)
    for a, b in zip(got, exp):
        assert len(a) == len(b) == len(HEADER)
        for x, y in zip(a, b):
            if y is None:
                assert x == "-", (a, b)
            elif isinstance(y, np.float64):
                assert np.float64(x) == y, (a, b)
            else:
                assert x == str(y), (a, b)


def test_profile_seam_fragments(world):
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng, ids, sp = world
    plain, wd = root / "wd_plain", root / "wd_fr"
    others = dict(read_strain_file="rs.tsv", strain_read_support_file="sup.tsv", strain_mosaic_file="mo.tsv")
    _profile(eng, db, plain, gaf, **{k: str(plain / v) for k, v in others.items()})
    _profile(eng, db, wd, gaf, strain_fragments_file=str(wd / "fr.tsv"), **{k: str(wd / v) for k, v in others.items()})
    for f in ("species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt") + tuple(others.values()):   # the option changes no other output
        assert open(wd / f, "rb").read() == open(plain / f, "rb").read(), f
    assert not os.path.exists(plain / "fr.tsv")
    rows = _lines(wd / "fr.tsv")
    assert rows[0] == HEADER
    # the candidates from the tables, as the read support report's test takes them: the rows of strain_abundance.txt, weight = predicted_coverage
    gi = _lines(db / "genomes_info.txt")[1:]
    genome_hap = {r[0]: r[0].split("_ASM")[0] for r in gi}
    names = [g.name for g in sset.species]
    S = len(names)
    table = _lines(wd / "strain_abundance.txt")[1:]
    cand = {s: [] for s in range(S)}
    for r in table:
        s = names.index(r[0])
        h = sset.species[s].hap_names.index(genome_hap[r[2]])
        if h not in [x[0] for x in cand[s]]:                                  # (a haplotype's first row stands for it)
            cand[s].append((h, float(r[3])))
    assert all(len(cand[s]) >= 2 for s in cand)
    for s in cand:
        cand[s].sort()                                                        # ascending haplotype index: the seam's candidate lists
    off = np.cumsum([0] + [len(cand[s]) for s in range(S)]).astype(np.uint64)
    ch = np.array([h for s in range(S) for h, _ in cand[s]], dtype=np.uint32)
    cw = np.array([w for s in range(S) for _, w in cand[s]], dtype=np.float64)
    entry = {(s, h): int(off[s]) + i for s in cand for i, (h, _) in enumerate(cand[s])}
    strain_rows = []
    for r in table:
        s = names.index(r[0])
        strain_rows.append((s, entry[(s, sset.species[s].hap_names.index(genome_hap[r[2]]))], r[1], r[2]))
    # the reference on the same selection: keys and tags of the ids, the duplicate-id rule on the whole ids, the reads as the oracle bins them
    kt = [ref.fragment_key(i.encode()) for i in ids]
    mate, counts = ref.fragment_mates([k for k, _ in kt], [t for _, t in kt])
    assert counts[0] > 500 and counts[1] > 100 and counts[2] >= 10 and counts[3] == 2
    species_of_id = {}
    for r, i in enumerate(ids):
        if sp[r] >= 0:
            species_of_id.setdefault(i, set()).add(int(sp[r]))
    flags = np.array([1 if sp[r] >= 0 and len(species_of_id[i]) > 1 else 0 for r, i in enumerate(ids)], dtype=np.uint8)
    assert flags.sum() >= 2
    _, read_rows = _rows(sset.species, sset.reads, flags)
    exp = ref.strain_fragments(_hap_nodes(sset.species), read_rows, off, ch, cw, mate)
    hap, species, status, pair_off, pair, _ = exp
    assert (species[:, [ref.PAIRED, ref.CONCORDANT, ref.SINGLE, ref.MULTI, ref.ELSEWHERE], 0] > 0).all() and hap[:, ref.UNIQUE_BY_PAIR, 0].sum() > 0
    seq = [names.index(r[0]) for r in _lines(wd / "sup.tsv")[1:] if r[3] == "counted"]   # the species in the order they went through the device
    assert sorted(seq) == list(range(S))
    _same_rows(rows[1:], ref.report_rows(names, strain_rows, seq, hap, species, status, pair_off, pair, off))
    # the stage calls on the same selection give the reference's numbers
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads, flags)
    eng.rcls_profile(want_species=False)
    got = eng.strain_fragments(off, ch, cw, mate)
    assert all(np.array_equal(g, e) for g, e in zip(got[:5], exp[:5]))
    full = open(wd / "fr.tsv", "rb").read()
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_fr_cli"
    wc.mkdir()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0",
                        "--strain-fragments", str(wc / "fr.tsv")], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc / "fr.tsv", "rb").read() == full
    # several ranks: refused with the table's wording
    wn = root / "wd_fr_ranks"
    with pytest.raises(PantaxHipError) as e:
        _profile(eng, db, wn, gaf, rank=0, world_size=2, allreduce=lambda buf: None, strain_fragments_file=str(wn / "fr.tsv"))
    assert e.value.code == E_INVALID and "the fragment support report (strain_fragments_file) needs one rank and an unsharded ingest (world_size 2)" in str(e.value)
    assert not os.path.exists(wn / "fr.tsv")
