"""GPU tests of the mosaic reads (pantax_hip_strain_mosaic, --strain-mosaic).  The expected integers come from the row-by-row reading of the contract in
tests/mosaic_ref.py (pinned by hand in tests/test_mosaic_ref.py); everything compares element for element."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import mosaic_ref as ref
from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile, seam_world

pytestmark = pytest.mark.gpu

_pop = lambda x: bin(x).count("1")


def _words(g, picks):
    """per species-local node the candidates that walk it, bit p = picks[p]"""
    words = [0] * g.n_nodes
    for p, h in enumerate(picks):
        for v in set(g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])].tolist()):
            words[v] |= 1 << p
    return words


def _compose(words, rng, seg_lens):
    """a walk (species-local nodes) whose greedy cut is exactly seg_lens: every segment stays inside the walk of one candidate, and the first node of the
    next segment is walked by nobody the segment has left"""
    live = [v for v in range(len(words)) if words[v]]
    walk, run = [], 0
    for j, ln in enumerate(seg_lens):
        pool = sorted((v for v in live if j == 0 or not (words[v] & run)), key=lambda v: _pop(words[v]))[:20]
        assert pool, "no node opens the next segment"
        v = pool[int(rng.integers(len(pool)))]
        walk.append(v)
        run = words[v]
        mine = [u for u in live if words[u] & (run & -run)]                # the nodes of one candidate of the segment
        for _ in range(ln - 1):
            some = [mine[int(i)] for i in rng.integers(len(mine), size=48)]
            u = min(some, key=lambda u: _pop(run & words[u])) if _pop(run) > 1 else some[0]
            walk.append(u)
            run &= words[u]
    return walk


def _members(words, nodes):
    return [set(p for p in range(words[v].bit_length()) if (words[v] >> p) & 1) for v in nodes]


def _k(words, nodes):
    """(k, foreign steps) of a walk by the reference's cut"""
    m = _members(words, nodes)
    empty = sum(1 for x in m if not x)
    return (0, empty) if empty else (len(ref.cut(m)), 0)


def _build():
    """Ten species as in the read support test: four tiny ones (their reads share one 64-step group with their neighbours'), K_s = 1, K_s = 2 with equal
    weights, a 64-haplotype species with all 64 as candidates (bit 63), a 70-haplotype species with 66 candidates (skipped), a species without candidates,
    and one that is left out of the db.  Short reads of the generator plus hand-placed walks composed from stretches of two or more candidates' walks."""
    import synthdata as synth
    rng = np.random.default_rng(8)
    shapes = [(2, 250), (3, 250), (2, 250), (3, 250), (1, 8000), (4, 8000), (64, 8000), (70, 8000), (3, 6000), (3, 6000)]
    species, start = [], 1
    for i, (H, glen) in enumerate(shapes):
        g = synth.make_species(rng, str(1000 + i), H, glen, start, "GCF_%06d" % (i + 1), present_frac=0.6)
        species.append(g)
        start = g.range_end + 1
    rd = synth.make_reads(rng, species[4:], 2500, adversarial_frac=0.0)
    picks = [[0, 1], [1], [], [2, 0, 1], [0], [2, 0], list(range(63, -1, -1)), sorted(rng.choice(70, size=66, replace=False).tolist()), []]
    weights = [[1.0, 2.0], [4.0], [], [3.0, 3.0, 3.0], [1.5], [2.5, 2.5], rng.choice([1.0, 2.5, 7.25], size=64).tolist(),
               (rng.random(66) * 10 + 0.1).tolist(), []]
    words = [_words(g, p) for g, p in zip(species, picks)]
    walks, ps, pe, sp_of, marks = [], [], [], [], {}

    def add(s, local_nodes, name=None, pstart=3, pend=40):
        if name:
            marks.setdefault(name, []).append(len(walks))
        walks.append(np.asarray(local_nodes, dtype=np.uint32) + np.uint32(species[s].range_start))
        ps.append(pstart)
        pe.append(pend)
        sp_of.append(s)

    def stretch(s, h, k, at=0):
        g = species[s]
        b = int(g.path_off[h])
        assert int(g.path_off[h + 1]) - b >= at + k
        return g.path_nodes[b + at:b + at + k].tolist()

    comp = lambda s, lens: _compose(words[s], rng, lens)
    for s in (0, 3, 0, 3):                                                  # two species with breaks inside one group
        add(s, comp(s, [2, 2]), "tiny")
    add(5, comp(5, [63, 1]), "lane63")                                      # 64 steps fill a group: a break at its last lane ...
    add(5, comp(5, [1, 63]), "lane1")                                       # ... and at its second
    add(5, comp(5, [1] * 64), "alternating")                                # 63 breaks: the round loop
    for s in (5, 6, 3):
        add(s, comp(s, [3, 4]), "k2")
        add(s, comp(s, [2, 2, 3]), "k3")
        add(s, comp(s, [2, 1, 3, 2]), "k4")
    add(5, comp(5, [64, 1]), "step64")                                      # 65 steps: the break exactly at step 64 ...
    add(5, comp(5, [63, 2]), "step63")                                      # ... at step 63 ...
    add(5, comp(5, [65, 65]), "step65")                                     # ... at step 65 of 130
    add(5, stretch(5, 2, 130, at=5), "long_compatible")                     # a segment that runs across the chunk borders without a break
    add(5, comp(5, [1] * 130), "long_alternating")                          # breaks in every chunk, at every lane
    add(5, comp(5, [20, 60, 50]), "long_three")
    add(6, comp(6, [70, 60]), "long_wide")
    foreign5 = [v for v in range(species[5].n_nodes) if not words[5][v]]
    assert len(foreign5) > 3
    w = comp(5, [2, 2])
    add(5, w[:1] + foreign5[:1] + w[1:] + foreign5[1:3], "foreign_short")   # a foreign step before and after the would-be break
    w = stretch(5, 0, 130, at=9)
    add(5, w[:129] + foreign5[:1], "foreign_long")                          # step 129: the third chunk, or the fourth
    foreign4 = [v for v in range(species[4].n_nodes) if not words[4][v]]
    add(4, stretch(4, 0, 3), "k1_compatible")
    if foreign4:
        add(4, stretch(4, 0, 2) + foreign4[:1], "k1_foreign")
    a, b = comp(5, [1, 1])
    add(5, [a, b, a], "revisit")                                            # a node on both sides of a break
    w = comp(5, [3, 4])
    for _ in range(3):
        add(5, w, "repeated")                                               # one junction three times
    add(7, comp(7, [3, 3]), "skipped")                                      # 66 candidates: counted only
    add(8, stretch(8, 0, 5), "no_candidates")
    add(5, comp(5, [2, 2]), "dropped")
    k = np.array([len(x) for x in walks], dtype=np.uint64)
    n = len(walks)
    one = lambda v: np.full(n, v, dtype=np.int64)
    reads = synth.PackedReads(np.concatenate([rd.step_off, rd.step_off[-1] + np.cumsum(k)]), np.concatenate([rd.node_id] + walks), None,
                              np.concatenate([rd.pstart, np.array(ps, dtype=np.int64)]), np.concatenate([rd.pend, np.array(pe, dtype=np.int64)]),
                              np.concatenate([rd.qlen, one(30000)]), np.concatenate([rd.mapq, one(60)]), np.concatenate([rd.plen, one(30000)]))
    R = reads.n_reads
    flags = np.zeros(R, dtype=np.uint8)
    hand0 = R - n
    flags[rng.choice(hand0, size=60, replace=False)] = rng.choice([1, 2], size=60).astype(np.uint8)
    flags[hand0 + marks["dropped"][0]] = 1                                  # a dropped mosaic read
    db = species[:9]                                                        # the last species is not in the db
    off = np.cumsum([0] + [len(x) for x in picks]).astype(np.uint64)
    cands = (off, np.array(sum(picks, []), dtype=np.uint32), np.array(sum(weights, []), dtype=np.float64))
    hand = {name: [(sp_of[i], (walks[i].astype(np.int64) - species[sp_of[i]].range_start).tolist()) for i in idx] for name, idx in marks.items()}
    return db, reads, flags, cands, words, hand


def _rows(db, reads, flags):
    from oracle import oracle as orc
    sp = orc.bin_reads(reads.step_off, reads.node_id, [g.range_start for g in db], [g.range_end for g in db])
    so = reads.step_off.astype(np.int64)
    rows = []
    for r in range(reads.n_reads):
        s = int(sp[r])
        nodes = (reads.node_id[so[r]:so[r + 1]].astype(np.int64) - db[s].range_start).tolist() if s >= 0 else []
        rows.append((s, flags[r] == 0, nodes, int(reads.pstart[r]), int(reads.pend[r])))
    return sp, rows


def _hap_nodes(db):
    return [[set(g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])].tolist()) for h in range(g.n_paths)] for g in db]


@pytest.fixture(scope="module")
def stage():
    from pantax_amd.engine import Engine
    db, reads, flags, cands, words, hand = _build()
    sp, rows = _rows(db, reads, flags)
    exp = ref.mosaic(_hap_nodes(db), rows, *cands)
    eng = Engine(0)
    eng.upload_db(db)
    eng.upload_reads(reads.step_off, reads.node_id, reads.pstart, reads.pend, reads.qlen, reads.mapq, flags)
    eng.rcls_profile(want_species=False)
    yield eng, db, reads, flags, cands, sp, exp, words, hand
    eng.close()


def _same(got, exp):
    assert len(got) == len(exp) == 8
    for g, e in zip(got[:7], exp[:7]):
        assert g.dtype == e.dtype and g.shape == e.shape
        assert np.array_equal(g, e)
    assert got[7] == exp[7]


def test_fixture_holds_the_cases(stage):
    """what the hand-placed walks are meant to be, asserted from the reference before anything is compared"""
    eng, db, reads, flags, cands, sp, exp, words, hand = stage
    species, extra, hap, pair_off, pair, jn, jc, total = exp
    ks = {name: [_k(words[s], nodes) for s, nodes in hand[name]] for name in hand if name not in ("skipped", "no_candidates")}
    assert ks["tiny"] == [(2, 0)] * 4 and {s for s, _ in hand["tiny"]} == {0, 3}
    assert ks["lane63"] == [(2, 0)] and ks["lane1"] == [(2, 0)] and len(hand["lane63"][0][1]) == len(hand["lane1"][0][1]) == 64
    assert ks["alternating"] == [(64, 0)] and len(hand["alternating"][0][1]) == 64
    assert ks["k2"] == [(2, 0)] * 3 and ks["k3"] == [(3, 0)] * 3 and ks["k4"] == [(4, 0)] * 3
    assert ks["step64"] == [(2, 0)] and ks["step63"] == [(2, 0)] and ks["step65"] == [(2, 0)] and ks["long_compatible"] == [(1, 0)]
    assert [len(hand[n][0][1]) for n in ("step64", "step63", "step65", "long_compatible", "long_alternating", "long_three", "long_wide")] == [65, 65, 130, 130, 130, 130, 130]
    assert ks["long_alternating"] == [(130, 0)] and ks["long_three"] == [(3, 0)] and ks["long_wide"] == [(2, 0)]
    assert ks["foreign_short"] == [(0, 3)] and ks["foreign_long"] == [(0, 1)] and ks["k1_compatible"] == [(1, 0)] and ks.get("k1_foreign", [(0, 1)]) == [(0, 1)]
    assert ks["revisit"] == [(3, 0)] and ks["repeated"] == [(2, 0)] * 3 and ks["dropped"] == [(2, 0)]
    s64, w64 = hand["step64"][0]
    assert [5, w64[63], w64[64]] in jn.tolist()                                       # a junction whose right node is step 64 of a long walk
    rep = hand["repeated"][0][1]
    assert jc[jn.tolist().index([5, rep[2], rep[3]])] >= 3 and len(set(jc[jn[:, 0] == 5].tolist())) >= 2   # distinct junctions of different counts
    assert (species[:, ref.MOSAIC1, 0] > 0).sum() >= 3 and species[5, ref.MOSAIC2, 0] > 0 and species[5, ref.MOSAIC3PLUS, 0] > 0 and species[6, ref.MOSAIC3PLUS, 0] > 0
    assert species[5, ref.FOREIGN, 0] >= 2 and extra[5, ref.FOREIGN_STEPS] >= 4
    m5 = pair[int(pair_off[5]):int(pair_off[6])].reshape(2, 2)
    assert m5[0, 1] > 60 and m5[1, 0] > 60 and m5[0, 0] == m5[1, 1] == 0               # a non-zero [a][b] and [b][a]
    assert species[2, 0, 0] == 0 and species[8, 0, 0] > 10 and not species[8, 1:].any() and species[7, 0, 0] > 10 and not species[7, 1:].any()
    assert pair_off[8] == pair_off[7] and pair_off[7] - pair_off[6] == 64 * 64        # 66 candidates: no block
    assert (sp < 0).sum() > 5 and ((sp >= 0) & (flags != 0)).sum() > 10               # "U" reads, dropped reads
    k = np.diff(reads.step_off.astype(np.int64))
    assert (k > 64).sum() >= 7 and (k == 64).sum() >= 3
    assert total == extra[:, ref.N_BREAKS].sum() > 200
    ref.check_identities(*exp[:7], cands[0])


def test_stage_call_equals_reference(stage, set_opt):
    eng, db, reads, flags, cands, sp, exp, words, hand = stage
    _same(eng.strain_mosaic(*cands), exp)
    set_opt(eng, "read_strain_route", "walk")                                        # every species through the compact walk masks
    _same(eng.strain_mosaic(*cands), exp)


def test_identities_and_read_support(stage):
    """the identities of the contract on the device's numbers, and the cross-identities against the read support pass on the same candidates"""
    eng, db, reads, flags, cands, sp, exp, words, hand = stage
    got = eng.strain_mosaic(*cands)
    _, sup_species, _, _ = eng.strain_read_support(*cands)
    ref.check_identities(*got[:7], cands[0], support_species=sup_species)
    assert np.array_equal(got[0][:, 0], sup_species[:, 0])                            # counted, also for K_s = 0 and K_s > 64


def _raw(eng, cands, n_species=None, pair_cap=None, junction_cap=0):
    from pantax_amd import _ffi
    from pantax_amd.engine import p
    off, ch, cw = cands
    S = eng.S
    cs = _ffi.ReadStrainSet(S if n_species is None else n_species, off.ctypes.data, ch.ctypes.data, cw.ctypes.data)
    k = np.diff(off.astype(np.int64))
    n_pair = int((k[k <= 64] ** 2).sum())
    out = dict(species=np.full((S, 6, 3), 77, dtype=np.uint64), extra=np.full((S, 3), 77, dtype=np.uint64), hap=np.full((len(ch), 2), 77, dtype=np.uint64),
               pair_off=np.full(S + 1, 77, dtype=np.uint64), pair=np.full(max(n_pair, 1), 77, dtype=np.uint64),
               jn=np.full((max(junction_cap, 1), 3), 77, dtype=np.uint32), jc=np.full(max(junction_cap, 1), 77, dtype=np.uint64))
    n_j, n_b = C.c_uint64(77), C.c_uint64(77)
    rc = eng.lib.pantax_hip_strain_mosaic(eng.ctx, eng.db, eng.reads, C.byref(cs), p(out["species"]), p(out["extra"]), p(out["hap"]), p(out["pair_off"]),
                                          n_pair if pair_cap is None else pair_cap, p(out["pair"]), junction_cap, p(out["jn"]), p(out["jc"]), C.byref(n_j), C.byref(n_b))
    return rc, out, int(n_j.value), int(n_b.value)


def test_junction_cap(stage):
    from pantax_amd import _ffi
    from pantax_amd._ffi import PantaxHipError
    eng, db, reads, flags, cands, sp, exp, words, hand = stage
    total = exp[7]
    # cap 0: not collected, the counters are the same
    got = eng.strain_mosaic(*cands, junction_cap=0)
    assert all(np.array_equal(g, e) for g, e in zip(got[:5], exp[:5])) and got[5].shape == (0, 3) and got[6].shape == (0,) and got[7] == total
    rc, out, n_j, n_b = _raw(eng, cands, junction_cap=0)
    assert rc == 0 and n_j == 0 and n_b == total and np.all(out["jn"] == 77) and np.all(out["jc"] == 77)
    assert np.array_equal(out["species"], exp[0]) and np.array_equal(out["pair"], exp[4])
    # one short of the breaks: E_LIMIT, the total (and the sizes) written, nothing else touched
    rc, out, n_j, n_b = _raw(eng, cands, junction_cap=total - 1)
    assert rc == _ffi.E_LIMIT and n_b == total and n_j == 77
    assert np.array_equal(out["pair_off"], exp[3])
    assert all(np.all(out[name] == 77) for name in ("species", "extra", "hap", "pair", "jn", "jc"))
    with pytest.raises(PantaxHipError) as e:
        eng.strain_mosaic(*cands, junction_cap=total - 1)
    assert e.value.code == _ffi.E_LIMIT
    # exactly the breaks: every junction fits (there are no more distinct junctions than breaks)
    rc, out, n_j, n_b = _raw(eng, cands, junction_cap=total)
    assert rc == 0 and n_b == total and n_j == len(exp[5])
    assert np.array_equal(out["jn"][:n_j], exp[5]) and np.array_equal(out["jc"][:n_j], exp[6]) and np.all(out["jn"][n_j:] == 77)
    _same(eng.strain_mosaic(*cands, junction_cap=total), exp)


def test_sizing_and_arguments(stage):
    from pantax_amd import _ffi
    from pantax_amd._ffi import PantaxHipError
    eng, db, reads, flags, cands, sp, exp, words, hand = stage
    rc, out, n_j, n_b = _raw(eng, cands, pair_cap=0)
    assert rc == _ffi.E_LIMIT
    assert np.array_equal(out["pair_off"], exp[3])                                    # the sizes are out ...
    assert all(np.all(out[name] == 77) for name in ("species", "extra", "hap", "pair", "jn", "jc")) and n_j == 77 and n_b == 77   # ... and nothing else is touched
    off, ch, cw = cands
    twice = ch.copy()
    twice[int(off[3]) + 1] = twice[int(off[3])]                                       # a haplotype twice within a species
    far = ch.copy()
    far[int(off[0])] = 2                                                              # species 0 has two haplotypes
    for bad in ((off, twice, cw), (off, far, cw)):
        with pytest.raises(PantaxHipError) as e:
            eng.strain_mosaic(*bad)
        assert e.value.code == -1
    assert _raw(eng, cands, n_species=eng.S + 1)[0] == -1


def test_empty_candidate_set(stage):
    eng, db, reads, flags, cands, sp, exp, words, hand = stage
    S = len(db)
    species, extra, hap, pair_off, pair, jn, jc, total = eng.strain_mosaic(np.zeros(S + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0))
    assert hap.shape == (0, 2) and pair.shape == (0,) and not pair_off.any() and jn.shape == (0, 3) and total == 0
    assert np.array_equal(species[:, 0], exp[0][:, 0]) and not species[:, 1:].any() and not extra.any()


def test_state(stage):
    """reads that are not binned, or binned against another db, are refused as by pantax_hip_strain_read_support"""
    from pantax_amd._ffi import PantaxHipError
    from pantax_amd.engine import Engine
    eng, db, reads, flags, cands, sp, exp, words, hand = stage
    with Engine(0) as e2:
        e2.upload_db(db)
        e2.upload_reads(reads.step_off, reads.node_id, reads.pstart, reads.pend, reads.qlen, reads.mapq, flags)
        with pytest.raises(PantaxHipError) as e:
            e2.strain_mosaic(*cands)                       # not binned yet
        assert e.value.code == -7
        e2.rcls_profile(want_species=False)
        e2.upload_db(db)                                   # a new db: the reads were binned against the previous one
        with pytest.raises(PantaxHipError) as e:
            e2.strain_mosaic(*cands)
        assert e.value.code == -7


# ---- the file seam -----------------------------------------------------------------------------------------------------------

HEADER = ["species_taxid", "strain_taxid", "genome_ID", "class", "n_reads", "n_steps", "span", "n_segments", "fraction", "other_strain_taxid", "other_genome_ID",
          "node_a", "node_b"]
CLASSES = ("counted", "compatible", "mosaic1", "mosaic2", "mosaic3plus", "foreign")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    yield from seam_world(tmp_path_factory, "pantax_mosaic", 37, 2, 5, 12000, 30000, present_frac=0.6, with_ids=True)


def _table_candidates(sset, db, wd):
    """the rows of strain_abundance.txt as candidate lists in ascending haplotype index: per species [(haplotype, weight, strain_taxid, genome_ID)]"""
    gi = _lines(db / "genomes_info.txt")[1:]
    genome_hap = {r[0]: r[0].split("_ASM")[0] for r in gi}
    names = [g.name for g in sset.species]
    table = _lines(wd / "strain_abundance.txt")[1:]
    cand = {s: [] for s in range(len(names))}
    for r in table:
        s = names.index(r[0])
        h = sset.species[s].hap_names.index(genome_hap[r[2]])
        if h not in [x[0] for x in cand[s]]:                          # (a haplotype's first row stands for it)
            cand[s].append((h, float(r[3]), r[1], r[2]))
    for s in cand:
        cand[s].sort()
    return names, table, genome_hap, cand


def _frac(n, of):
    return float(n) / float(of) if of else None


def test_profile_seam_mosaic(world, capfd, monkeypatch):
    import synthdata as synth
    from pantax_amd import _ffi
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf0, eng = world
    # the reported strains of the plain sample decide which walks are mosaic; those walks join the sample
    first = root / "wd_first"
    _profile(eng, db, first, gaf0)
    names, _, _, cand0 = _table_candidates(sset, db, first)
    assert all(len(cand0[s]) >= 2 for s in cand0)
    rng = np.random.default_rng(3)
    walks = []
    for s, g in enumerate(sset.species):
        words = _words(g, [h for h, _, _, _ in cand0[s]])
        one = _compose(words, rng, [3, 4])
        for lens, times in (([2, 2, 2], 4), ([2, 1, 2, 2], 1), ([40, 30], 1)):
            for _ in range(times):
                walks.append(np.asarray(_compose(words, rng, lens), dtype=np.uint32) + np.uint32(g.range_start))
        for _ in range(4 + s):
            walks.append(np.asarray(one, dtype=np.uint32) + np.uint32(g.range_start))                 # one junction several times
    rd = sset.reads
    k = np.array([len(w) for w in walks], dtype=np.uint64)
    n = len(walks)
    one = lambda v: np.full(n, v, dtype=np.int64)
    reads = synth.PackedReads(np.concatenate([rd.step_off, rd.step_off[-1] + np.cumsum(k)]), np.concatenate([rd.node_id] + walks),
                              np.concatenate([rd.strand, np.zeros(int(k.sum()), dtype=np.uint8)]), np.concatenate([rd.pstart, one(5)]), np.concatenate([rd.pend, one(140)]),
                              np.concatenate([rd.qlen, one(150)]), np.concatenate([rd.mapq, one(60)]), np.concatenate([rd.plen, one(150)]),
                              list(rd.read_id) + ["MOSAIC%d/1" % i for i in range(n)])
    gaf = root / "with_mosaic.gaf"
    synth.write_gaf(reads, str(gaf))
    plain = root / "wd_plain"
    _profile(eng, db, plain, gaf)
    wd = root / "wd_mo"
    _profile(eng, db, wd, gaf, strain_mosaic_file=str(wd / "mo.tsv"))
    for f in ("species_abundance.txt", "strain_abundance.txt"):       # the option changes none of the tables
        assert open(wd / f, "rb").read() == open(plain / f, "rb").read()
    assert not os.path.exists(plain / "mo.tsv")
    rows = _lines(wd / "mo.tsv")
    assert rows[0] == HEADER and all(len(r) == len(HEADER) for r in rows)
    body = rows[1:]
    names, table, genome_hap, cand = _table_candidates(sset, db, wd)
    assert all(len(cand[s]) >= 2 for s in cand)
    S = len(names)
    off = np.cumsum([0] + [len(cand[s]) for s in range(S)]).astype(np.uint64)
    ch = np.array([h for s in range(S) for h, _, _, _ in cand[s]], dtype=np.uint32)
    cw = np.array([w for s in range(S) for _, w, _, _ in cand[s]], dtype=np.float64)
    _, read_rows = _rows(sset.species, reads, np.zeros(reads.n_reads, dtype=np.uint8))
    species, extra, hap, pair_off, pair, jn, jc, total = ref.mosaic(_hap_nodes(sset.species), read_rows, off, ch, cw)
    assert all(species[s, ref.MOSAIC1, 0] > 0 and species[s, ref.MOSAIC2, 0] > 0 and species[s, ref.MOSAIC3PLUS, 0] > 0 for s in range(S)) and total > 10
    cell = lambda x: "-" if x is None else x
    exp = []
    # 1. the donor rows in the order of strain_abundance.txt
    entry = {(s, h): int(off[s]) + i for s in cand for i, (h, _, _, _) in enumerate(cand[s])}
    for r in table:
        s = names.index(r[0])
        e = entry[(s, sset.species[s].hap_names.index(genome_hap[r[2]]))]
        steps = int(species[s, ref.MOSAIC1:ref.FOREIGN, 1].sum())
        exp.append([r[0], r[1], r[2], "donor", None, int(hap[e, 1]), None, int(hap[e, 0]), _frac(hap[e, 1], steps), None, None, None, None])
    # 2. the species rows in shard order
    for s in range(S):
        for j, cls in enumerate(CLASSES):
            q = species[s, j].tolist()
            exp.append([names[s], None, None, cls] + q + [int(extra[s, 2]) if cls == "foreign" else None, _frac(q[0], species[s, 0, 0]), None, None, None, None])
        q = species[s, ref.MOSAIC1:ref.FOREIGN].sum(axis=0).tolist()
        exp.append([names[s], None, None, "mosaic_total"] + q + [int(extra[s, 0]), _frac(q[0], species[s, 0, 0]), None, None, None, None])
    # 3. the switches of every pair of rows a < b
    n_switch = 0
    for s in range(S):
        K = len(cand[s])
        m = pair[int(pair_off[s]):int(pair_off[s + 1])].reshape(K, K)
        for a in range(K):
            for b in range(a + 1, K):
                if m[a, b] + m[b, a]:
                    n_switch += 1
                    exp.append([names[s], cand[s][a][2], cand[s][a][3], "switch", None, None, None, int(m[a, b] + m[b, a]), _frac(m[a, b] + m[b, a], extra[s, 1]),
                                cand[s][b][2], cand[s][b][3], None, None])
    # 4. the junctions, ten a species by default
    def junction_rows(top):
        out = []
        for s in range(S):
            for i in ref.top(jn, jc, s, top):
                out.append([names[s], None, None, "junction", None, None, None, int(jc[i]), _frac(jc[i], extra[s, 1]), None, None,
                            int(jn[i, 1]) + sset.species[s].range_start, int(jn[i, 2]) + sset.species[s].range_start])
        return out
    assert n_switch > 0 and max(jc.tolist()) >= 4 and all((jn[:, 0] == s).sum() > 10 for s in range(S))

    def check(body, exp):
        assert len(body) == len(exp)
        for row, e in zip(body, exp):
            for i, (got, want) in enumerate(zip(row, e)):
                if want is None:
                    assert got == "-", (row, e)
                elif isinstance(want, float):
                    assert float(got) == want, (row, e)
                else:
                    assert got == str(want), (row, e)
    check(body, exp + junction_rows(10))
    full = open(wd / "mo.tsv", "rb").read()
    # --strain-mosaic-top 1 and off
    w1 = root / "wd_mo_top1"
    _profile(eng, db, w1, gaf, strain_mosaic_file=str(w1 / "mo.tsv"), strain_mosaic_top=1)
    check(_lines(w1 / "mo.tsv")[1:], exp + junction_rows(1))
    woff = root / "wd_mo_off"
    _profile(eng, db, woff, gaf, strain_mosaic_file=str(woff / "mo.tsv"), strain_mosaic_top="off")
    check(_lines(woff / "mo.tsv")[1:], exp)
    # a species-only run writes nothing; the strain-only resume behind it writes the same file
    wr = root / "wd_mo_resume"
    capfd.readouterr()
    _profile(eng, db, wr, gaf, species=True, strain=False, out_binning_file=str(wr / "reads_classification.tsv"), strain_mosaic_file=str(wr / "mo_species_only.tsv"))
    assert not os.path.exists(wr / "mo_species_only.tsv") and "no strain step" in capfd.readouterr().err
    _profile(eng, db, wr, gaf, species=False, strain=True, strain_mosaic_file=str(wr / "mo.tsv"))
    assert open(wr / "mo.tsv", "rb").read() == full
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_mo_cli"
    wc.mkdir()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0",
                        "--strain-mosaic", str(wc / "mo.tsv"), "--strain-mosaic-top", "off"], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc / "mo.tsv", "rb").read() == open(woff / "mo.tsv", "rb").read()
    # several ranks: refused on every rank with the table's wording, before any collective
    for rank in range(2):
        wn = root / ("wd_mo_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, strain_mosaic_file=str(wn / "mo.tsv"))
        assert e.value.code == -1 and "the mosaic read report (strain_mosaic_file) needs one rank and an unsharded ingest (world_size 2)" in str(e.value)
        assert not os.path.exists(wn / "mo.tsv")
    # a caller compiled against the header before these fields: its struct ends behind strain_segments_peak, the report reads as off
    real = _ffi.ProfileExt

    class OldExt(real):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.struct_size = 120

    monkeypatch.setattr(_ffi, "ProfileExt", OldExt)
    wold = root / "wd_mo_old"
    _profile(eng, db, wold, gaf, strain_fit_file=str(wold / "fit.tsv"), strain_mosaic_file=str(wold / "mo.tsv"))
    monkeypatch.setattr(_ffi, "ProfileExt", real)
    assert os.path.exists(wold / "fit.tsv") and not os.path.exists(wold / "mo.tsv")
    assert open(wold / "strain_abundance.txt", "rb").read() == open(wd / "strain_abundance.txt", "rb").read()
