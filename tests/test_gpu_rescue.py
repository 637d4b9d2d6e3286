"""GPU tests of the read rescue (pantax_hip_strain_read_rescue, --strain-rescue).  The expected integers come from the row-by-row reading of the contract
in tests/rescue_ref.py (pinned by hand in tests/test_rescue_ref.py); everything compares element for element."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import rescue_ref as ref
from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile, seam_world
from tests.near_miss_ref import near_miss_rank

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -7


def _members(g, haps):
    """per species-local node the positions of `haps` whose walk visits it"""
    out = [set() for _ in range(g.n_nodes)]
    for p, h in enumerate(haps):
        for v in set(g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])].tolist()):
            out[v].add(p)
    return out


def _build():
    """Ten species as in the mosaic test: four tiny ones (their reads share one 64-step group with their neighbours'), K_s = 0 with a candidate, a
    4-haplotype species with two reported and two candidates (the hand-placed walks), a 64-haplotype species with K_s + J_s = 64 (bit 63), a
    70-haplotype species with K_s + J_s = 66 (skipped), a species of K_s = J_s = 1 with a haplotype in neither list (novel nodes), and one that is left
    out of the db.  J_s = 0 is tiny species 1.  Short reads of the generator plus walks composed node by node from the membership of every node."""
    import synthdata as synth
    rng = np.random.default_rng(8)
    shapes = [(2, 250), (3, 250), (2, 250), (3, 250), (1, 8000), (4, 8000), (64, 8000), (70, 8000), (3, 6000), (3, 6000)]
    species, start = [], 1
    for i, (H, glen) in enumerate(shapes):
        g = synth.make_species(rng, str(1000 + i), H, glen, start, "GCF_%06d" % (i + 1), present_frac=0.6)
        species.append(g)
        start = g.range_end + 1
    rd = synth.make_reads(rng, species[4:], 2500, adversarial_frac=0.0)
    wide = rng.permutation(70)[:66].tolist()
    sel = [[0], [1], [0], [2, 0], [], [3, 2], list(range(63, 23, -1)), wide[:30], [0]]
    cand = [[1], [], [1], [1], [0], [1, 0], list(range(24)), wide[30:], [1]]
    M = [_members(g, x) for g, x in zip(species, sel)]
    N = [_members(g, x) for g, x in zip(species, cand)]
    walks, ps, pe, sp_of, marks = [], [], [], [], {}

    def add(s, local_nodes, name, pstart=3, pend=40):
        marks.setdefault(name, []).append(len(walks))
        walks.append(np.asarray(local_nodes, dtype=np.uint32) + np.uint32(species[s].range_start))
        ps.append(pstart)
        pe.append(pend)
        sp_of.append(s)

    def pool(s, pred):
        out = [v for v in range(species[s].n_nodes) if pred(M[s][v], N[s][v])]
        assert out, "no such node in species %d" % s
        return out

    def fill(nodes, n):
        return [nodes[i % len(nodes)] for i in range(n)]

    # species 5: Sel = [3, 2] (positions 0, 1), Cand = [1, 0] (positions 0, 1): haplotypes 0 and 1 share a clade, and so do 2 and 3
    both = pool(5, lambda m, n: m and n == {0, 1})                         # reported, and walked by both candidates
    c0_only = pool(5, lambda m, n: m and n == {0})                         # reported, candidate 0 but not candidate 1
    f_both = pool(5, lambda m, n: not m and n == {0, 1})                   # foreign steps ...
    f_c0 = pool(5, lambda m, n: not m and n == {0})
    f_c1 = pool(5, lambda m, n: not m and n == {1})
    a_only = pool(5, lambda m, n: m == {0} and 0 in n)                     # one reported strain each, candidate 0 walks both
    b_only = pool(5, lambda m, n: m == {1} and 0 in n)
    a_bare = pool(5, lambda m, n: m == {0} and not n)                      # ... and no candidate walks this one
    core = pool(5, lambda m, n: m == {0, 1})
    add(5, core[:3], "compatible")
    add(5, [a_only[0], b_only[0]], "mosaic_rescued")
    add(5, [a_bare[0], b_only[0]], "mosaic_unrescued")
    add(5, [c0_only[0], f_c0[0]], "foreign_rescued")
    add(5, [f_c0[0], f_c1[0]], "foreign_patchwork")
    add(5, [f_both[0], both[0]], "contested")
    add(5, [f_both[0], f_both[0], both[0]], "revisit")                      # a node twice: two foreign steps
    add(5, [a_only[0], b_only[0]], "dropped")
    add(5, f_both[:1] + fill(both, 63), "lane0")                           # 64 steps fill a group: the only foreign step at its first lane ...
    add(5, fill(both, 63) + f_both[:1], "lane63")                          # ... and at its last
    add(5, f_c0[:1] + fill(c0_only, 64), "long65_first")                   # 65 steps: the foreign step first, and at step 64 = last
    add(5, fill(c0_only, 64) + f_c0[:1], "long65_last")
    add(5, f_c0[:1] + fill(c0_only, 129), "long130_first")                 # 130 steps: first, step 64, last (the third chunk); rescued by one
    add(5, fill(c0_only, 64) + f_c0[:1] + fill(c0_only, 65), "long130_step64")
    add(5, fill(c0_only, 129) + f_c0[:1], "long130_last")
    add(5, fill(both, 100) + f_both[:1] + fill(both, 29), "long_contested")  # rescued by two
    add(5, fill(both, 70) + f_c0[:1] + fill(both, 58) + f_c1[:1], "long_patchwork")
    add(5, fill(a_only, 70) + fill(b_only, 60), "long_mosaic_rescued")
    add(5, fill(core, 130), "long_compatible")
    # species 8: Sel = [0], Cand = [1], haplotype 2 in neither list
    nobody = pool(8, lambda m, n: not m and not n)
    mine = pool(8, lambda m, n: m and n)
    add(8, [mine[0], nobody[0]], "foreign_novel")
    add(8, fill(mine, 100) + nobody[:1] + fill(mine, 29), "long_novel")
    # the four tiny species: short walks that share one group
    for s in (0, 1, 2, 3, 0, 1, 2, 3):
        add(s, list(range(min(3, species[s].n_nodes))), "tiny")
    add(4, list(range(4)), "k0")
    add(6, pool(6, lambda m, n: True)[:5], "wide64")
    add(7, list(range(5)), "skipped")
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
    flags[hand0 + marks["dropped"][0]] = 1
    db = species[:9]                                                        # the last species is not in the db
    u64, u32 = lambda x: np.array(x, dtype=np.uint64), lambda x: np.array(x, dtype=np.uint32)
    sets = (u64(np.cumsum([0] + [len(x) for x in sel])), u32(sum(sel, [])), u64(np.cumsum([0] + [len(x) for x in cand])), u32(sum(cand, [])))
    hand = {name: [(sp_of[i], (walks[i].astype(np.int64) - species[sp_of[i]].range_start).tolist()) for i in idx] for name, idx in marks.items()}
    return db, reads, flags, sets, (M, N), hand


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


def _fixture_holds_the_cases(db, reads, flags, sets, MN, hand, sp, exp):
    """what the hand-placed walks are meant to be and that no class is empty, from the reference alone: a set that leaves a class empty hides a failure"""
    M, N = MN
    species, step, cand, cand_steps = exp
    out = {name: [ref.walk([M[s][v] for v in nodes], [N[s][v] for v in nodes]) for s, nodes in hand[name]] for name in hand if name != "skipped"}
    cls = lambda name: [o[0] for o in out[name]]
    assert cls("compatible") == [ref.W_COMPATIBLE] and cls("long_compatible") == [ref.W_COMPATIBLE]
    assert cls("mosaic_rescued") == [ref.W_MOSAIC_RESCUED] and out["mosaic_rescued"][0][1] and cls("long_mosaic_rescued") == [ref.W_MOSAIC_RESCUED]
    assert cls("mosaic_unrescued") == [ref.W_MOSAIC_UNRESCUED] and cls("dropped") == [ref.W_MOSAIC_RESCUED]
    assert cls("foreign_rescued") == [ref.W_FOREIGN_RESCUED] and out["foreign_rescued"][0][1] == {0}
    assert cls("foreign_patchwork") == [ref.W_FOREIGN_PATCHWORK] and out["foreign_patchwork"][0][2] == [2, 2, 0]
    assert cls("foreign_novel") == [ref.W_FOREIGN_NOVEL] and out["foreign_novel"][0][2] == [1, 0, 1]
    assert cls("contested") == [ref.W_FOREIGN_RESCUED] and out["contested"][0][1] == {0, 1} and out["revisit"][0][2] == [2, 2, 0]
    for name in ("lane0", "lane63"):
        assert len(hand[name][0][1]) == 64 and out[name] == [(ref.W_FOREIGN_RESCUED, {0, 1}, [1, 1, 0])]
    assert not M[5][hand["lane0"][0][1][0]] and not M[5][hand["lane63"][0][1][63]]
    for name, n, at in (("long65_first", 65, 0), ("long65_last", 65, 64), ("long130_first", 130, 0), ("long130_step64", 130, 64), ("long130_last", 130, 129)):
        nodes = hand[name][0][1]
        assert len(nodes) == n and [i for i, v in enumerate(nodes) if not M[5][v]] == [at] and out[name] == [(ref.W_FOREIGN_RESCUED, {0}, [1, 1, 0])]
    assert out["long_contested"] == [(ref.W_FOREIGN_RESCUED, {0, 1}, [1, 1, 0])] and len(hand["long_contested"][0][1]) == 130
    assert out["long_patchwork"] == [(ref.W_FOREIGN_PATCHWORK, set(), [2, 2, 0])] and len(hand["long_patchwork"][0][1]) == 130
    assert out["long_novel"] == [(ref.W_FOREIGN_NOVEL, set(), [1, 0, 1])] and len(hand["long_novel"][0][1]) == 130
    assert {s for s, _ in hand["tiny"]} == {0, 1, 2, 3} and sum(len(nodes) for _, nodes in hand["tiny"]) <= 64
    K, J = np.diff(sets[0].astype(np.int64)), np.diff(sets[2].astype(np.int64))
    assert K[4] == 0 and J[4] == 1 and J[1] == 0 and K[6] + J[6] == 64 and K[7] + J[7] == 66 and 63 in sets[1][int(sets[0][6]):int(sets[0][7])].tolist()
    assert (species[:, :, 0].sum(axis=0) > 0).all()                                                    # every one of the nine classes holds a read ...
    assert (np.delete(species[5, :, 0], ref.FOREIGN_NOVEL) > 0).all() and species[8, ref.FOREIGN_NOVEL, 0] >= 2   # ... species 5 all but novel, which species 8 holds
    assert (species[[0, 1, 2, 3], ref.COUNTED, 0] == 2).all() and species[4, ref.COUNTED, 0] > 10 and np.array_equal(species[4, ref.FOREIGN], species[4, ref.COUNTED])
    assert species[6, ref.COUNTED, 0] > 10 and species[7, ref.COUNTED, 0] > 10 and not species[7, 1:].any() and not step[7].any()
    assert (cand[int(sets[2][5]):int(sets[2][6]), ref.ALONE, 0] > 0).all() and (cand_steps[int(sets[2][5]):int(sets[2][6])] > 0).all()
    assert (sp < 0).sum() > 5 and ((sp >= 0) & (flags != 0)).sum() > 10                                # "U" reads, dropped reads
    k = np.diff(reads.step_off.astype(np.int64))
    assert (k > 64).sum() >= 10 and (k == 64).sum() >= 2
    ref.check_identities(*exp, sets[0], sets[2])


@pytest.fixture(scope="module")
def stage():
    from pantax_amd.engine import Engine
    db, reads, flags, sets, MN, hand = _build()
    sp, rows = _rows(db, reads, flags)
    exp = ref.rescue(_hap_nodes(db), rows, *sets)
    _fixture_holds_the_cases(db, reads, flags, sets, MN, hand, sp, exp)      # on the CPU, before any GPU run
    eng = Engine(0)
    eng.upload_db(db)
    eng.upload_reads(reads.step_off, reads.node_id, reads.pstart, reads.pend, reads.qlen, reads.mapq, flags)
    eng.rcls_profile(want_species=False)
    yield eng, db, reads, flags, sets, exp
    eng.close()


def _same(got, exp):
    assert len(got) == len(exp) == 4
    for g, e in zip(got, exp):
        assert g.dtype == e.dtype == np.uint64 and g.shape == e.shape
        assert np.array_equal(g, e)


def test_stage_call_equals_reference(stage, set_opt):
    eng, db, reads, flags, sets, exp = stage
    _same(eng.strain_read_rescue(*sets), exp)
    set_opt(eng, "read_strain_route", "walk")                                        # every species through the compact walk masks
    _same(eng.strain_read_rescue(*sets), exp)


def test_identities_and_cross_identities(stage):
    """the identities of the contract on the device's numbers, and the three cross-identities against the mosaic and the read support pass"""
    eng, db, reads, flags, sets, exp = stage
    species, step, cand, cand_steps = eng.strain_read_rescue(*sets)
    ref.check_identities(species, step, cand, cand_steps, sets[0], sets[2])
    so, sh, co, ch = sets
    S = len(db)
    K, J = np.diff(so.astype(np.int64)), np.diff(co.astype(np.int64))
    mo_species, mo_extra = eng.strain_mosaic(so, sh, np.arange(len(sh), dtype=np.float64), junction_cap=0)[:2]   # cand = Sel, whatever the weights
    lst, off = [], [0]
    for s in range(S):
        lst += sh[int(so[s]):int(so[s + 1])].tolist() + ch[int(co[s]):int(co[s + 1])].tolist()
        off.append(len(lst))
    sup_species = eng.strain_read_support(np.array(off, dtype=np.uint64), np.array(lst, dtype=np.uint32), np.ones(len(lst)))[1]
    checked = 0
    for s in range(S):
        assert np.array_equal(species[s, ref.COUNTED], mo_species[s, 0]) and np.array_equal(species[s, ref.COUNTED], sup_species[s, 0])
        if K[s] + J[s] > 64:
            continue
        if K[s] >= 1:
            assert np.array_equal(species[s, ref.COMPATIBLE], mo_species[s, 1]) and np.array_equal(species[s, ref.FOREIGN], mo_species[s, 5])
            assert np.array_equal(species[s, ref.MOSAIC], mo_species[s, 2:5].sum(axis=0)) and step[s, ref.FOREIGN_STEPS] == mo_extra[s, 2]
        if K[s] + J[s] >= 1:
            explained = species[s, ref.COMPATIBLE] + species[s, ref.FOREIGN_RESCUED] + species[s, ref.MOSAIC_RESCUED]
            assert np.array_equal(explained, sup_species[s, 0] - sup_species[s, 1])
            checked += 1
    assert checked >= 7


def _raw(eng, sets, n_species=None):
    from pantax_amd import _ffi
    from pantax_amd.engine import p
    so, sh, co, ch = [np.ascontiguousarray(x) for x in sets]
    S = eng.S
    cs = _ffi.NearMissSet(S if n_species is None else n_species, so.ctypes.data, sh.ctypes.data, co.ctypes.data, ch.ctypes.data)
    out = [np.full((S, 9, 3), 77, dtype=np.uint64), np.full((S, 3), 77, dtype=np.uint64), np.full((max(len(ch), 1), 3, 3), 77, dtype=np.uint64),
           np.full(max(len(ch), 1), 77, dtype=np.uint64)]
    rc = eng.lib.pantax_hip_strain_read_rescue(eng.ctx, eng.db, eng.reads, C.byref(cs), p(out[0]), p(out[1]), p(out[2]), p(out[3]))
    return rc, out


def test_arguments(stage):
    """the argument errors of pantax_hip_strain_near_miss, with the outputs left as given"""
    eng, db, reads, flags, sets, exp = stage
    so, sh, co, ch = sets
    rc, out = _raw(eng, sets)
    assert rc == 0 and all(np.array_equal(o[:len(e)], e) for o, e in zip(out, exp))
    twice_sel, twice_cand, far, shared = sh.copy(), ch.copy(), ch.copy(), ch.copy()
    twice_sel[int(so[5]) + 1] = twice_sel[int(so[5])]                                 # a haplotype twice within Sel_s ...
    twice_cand[int(co[5]) + 1] = twice_cand[int(co[5])]                               # ... within Cand_s
    far[int(co[0])] = 2                                                               # species 0 has two haplotypes
    shared[int(co[5])] = sh[int(so[5])]                                               # a haplotype in both
    for bad, kw in (((so, twice_sel, co, ch), {}), ((so, sh, co, twice_cand), {}), ((so, sh, co, far), {}), ((so, sh, co, shared), {}),
                    ((so[:-1], sh, co[:-1], ch), {"n_species": eng.S - 1})):
        rc, out = _raw(eng, bad, **kw)
        assert rc == E_INVALID and all(np.all(o == 77) for o in out), bad


def test_empty_sets(stage):
    """K_s = J_s = 0 everywhere: every species is open, every counted read is foreign and novel"""
    eng, db, reads, flags, sets, exp = stage
    S = len(db)
    z = np.zeros(S + 1, dtype=np.uint64)
    species, step, cand, cand_steps = eng.strain_read_rescue(z, np.zeros(0, dtype=np.uint32), z, np.zeros(0, dtype=np.uint32))
    assert cand.shape == (0, 3, 3) and cand_steps.shape == (0,)
    assert np.array_equal(species[:, ref.COUNTED], exp[0][:, ref.COUNTED])
    assert np.array_equal(species[:, ref.FOREIGN], species[:, ref.COUNTED]) and np.array_equal(species[:, ref.FOREIGN_NOVEL], species[:, ref.COUNTED])
    assert not species[:, [ref.COMPATIBLE, ref.FOREIGN_RESCUED, ref.FOREIGN_PATCHWORK, ref.MOSAIC, ref.MOSAIC_RESCUED, ref.CONTESTED]].any()
    assert np.array_equal(step[:, ref.FOREIGN_STEPS], species[:, ref.COUNTED, 1]) and np.array_equal(step[:, ref.NOVEL_STEPS], step[:, ref.FOREIGN_STEPS])


def test_state(stage):
    """reads that are not binned, or binned against another db, are refused as by pantax_hip_strain_read_support; the outputs are left as given"""
    from pantax_amd._ffi import PantaxHipError
    from pantax_amd.engine import Engine
    eng, db, reads, flags, sets, exp = stage
    with Engine(0) as e2:
        e2.upload_db(db)
        e2.upload_reads(reads.step_off, reads.node_id, reads.pstart, reads.pend, reads.qlen, reads.mapq, flags)
        with pytest.raises(PantaxHipError) as e:
            e2.strain_read_rescue(*sets)                   # not binned yet
        assert e.value.code == E_STATE
        rc, out = _raw(e2, sets)
        assert rc == E_STATE and all(np.all(o == 77) for o in out)
        e2.rcls_profile(want_species=False)
        e2.upload_db(db)                                   # a new db: the reads were binned against the previous one
        with pytest.raises(PantaxHipError) as e:
            e2.strain_read_rescue(*sets)
        assert e.value.code == E_STATE


def test_host_helpers_through_the_binding():
    """rescue_walk and rescue_rank of the engine module against the reference (the native check holds their edges)"""
    from pantax_amd.engine import rescue_rank, rescue_walk
    cls, d, steps = rescue_walk([2, 0], [1, 3], 2, 2)
    assert (cls, d, steps.tolist()) == (ref.W_FOREIGN_RESCUED, 1, [1, 1, 0])
    cls, d, steps = rescue_walk([1, 2], [0, 1], 2, 2)
    assert (cls, d, steps.tolist()) == (ref.W_MOSAIC_UNRESCUED, 0, [0, 0, 0])
    with pytest.raises(ValueError):
        rescue_walk([1], [1], 33, 32)
    cand = np.zeros((3, 3, 3), dtype=np.uint64)
    cand[0, 0] = [1, 5, 10]
    cand[2, 0] = [2, 2, 10]
    assert rescue_rank([4, 5, 6], cand).tolist() == ref.rank([4, 5, 6], cand) == [2, 0]
    assert rescue_rank([4, 5, 6], cand, top=1).tolist() == [2]


# ---- the file seam -----------------------------------------------------------------------------------------------------------

HEADER = ["species_taxid", "strain_taxid", "genome_ID", "rank", "class", "n_reads", "n_steps", "span", "fraction", "alone_reads", "foreign_reads", "foreign_steps",
          "claimed_steps", "stage", "unique_trio_nodes_fraction"]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    yield from seam_world(tmp_path_factory, "pantax_rescue", 32, 3, 5, 9000, 30000, present_frac=0.6, with_ids=True)


def _frac(n, of):
    return np.float64(n) / np.float64(of) if int(of) else None


def _expected_rows(sset, db, wd, eng, top):
    """the report from the reference and the run's tables: Sel = the rows of strain_abundance.txt, Cand = every other haplotype (the world's species are
    narrow) in the order of the near-miss rank, then ascending; the stage and the fraction from ori_strain_abundance.txt"""
    table = _lines(wd / "strain_abundance.txt")[1:]
    ori = {(r[0], r[2]): r for r in _lines(wd / "ori_strain_abundance.txt")[1:]}
    names = [g.name for g in sset.species]
    genomes = _lines(db / "genomes_info.txt")[1:]
    col = {c: i for i, c in enumerate(_lines(db / "genomes_info.txt")[0])}
    genome_of = {}
    for r in genomes:
        genome_of.setdefault(r[0].split("_ASM")[0], r)                       # the first row of every haplotype
    hap_of_genome = {r[0]: r[0].split("_ASM")[0] for r in genomes}
    S = len(names)
    reported = [set() for _ in names]
    for t in table:
        reported[names.index(t[0])].add(sset.species[names.index(t[0])].hap_names.index(hap_of_genome[t[2]]))
    u64, u32 = lambda x: np.array(x, dtype=np.uint64), lambda x: np.array(x, dtype=np.uint32)
    sel = [sorted(reported[s]) for s in range(S)]
    rest = [[h for h in range(sset.species[s].n_paths) if h not in reported[s]] for s in range(S)]
    so, sh = u64(np.cumsum([0] + [len(x) for x in sel])), u32(sum(sel, []))
    ro, rh = u64(np.cumsum([0] + [len(x) for x in rest])), u32(sum(rest, []))
    nm_cand, _ = eng.strain_near_miss(so, sh, ro, rh)                        # (pinned against its own reference in the near-miss tests)
    cand = []
    for s in range(S):
        c0, c1 = int(ro[s]), int(ro[s + 1])
        first = [rest[s][c] for c in near_miss_rank(rh[c0:c1], nm_cand[c0:c1], 0)]
        cand.append(first + [h for h in rest[s] if h not in first])
    assert any(c != sorted(c) for c in cand)                                 # the rank order is not the ascending one somewhere
    co, ch = u64(np.cumsum([0] + [len(x) for x in cand])), u32(sum(cand, []))
    _, read_rows = _rows(sset.species, sset.reads, np.zeros(sset.reads.n_reads, dtype=np.uint8))
    species, step, cd, cd_steps = ref.rescue(_hap_nodes(sset.species), read_rows, so, sh, co, ch)
    seq = [r[0] for r in _lines(wd / "ev.tsv")[1:] if r[3] == "total"]       # the species that went through the strain step, in the run's order
    assert len(set(seq)) == len(seq) >= 2 and {t[0] for t in table} <= set(seq)
    rows = []
    for x in seq:
        s = names.index(x)
        c0, c1 = int(co[s]), int(co[s + 1])
        for k, c in enumerate(ref.rank(ch[c0:c1], cd[c0:c1], top)):
            h = int(ch[c0 + c])
            g = genome_of.get(sset.species[s].hap_names[h])
            o = ori.get((names[s], g[0] if g else ""))
            assert o is not None
            stage = "first_filter" if o[8] == "" else ("second_filter" if o[3] == "" else "table_filter")
            q = cd[c0 + c]
            rows.append([x, g[col["strain_taxid"]] if g else "", g[0] if g else "", k + 1, "candidate"] + q[ref.RESCUED].tolist() +
                        [_frac(q[ref.RESCUED, 0], species[s, ref.FOREIGN, 0] + species[s, ref.MOSAIC, 0]), int(q[ref.ALONE, 0]), int(q[ref.FROM_FOREIGN, 0]), None,
                         int(cd_steps[c0 + c]), stage, np.float64(o[6]) if o[6] else None])
    for x in seq:
        s = names.index(x)
        for j, cls in enumerate(ref.NAMES):
            fs = [int(step[s, 0]), int(step[s, 1])] if cls == "foreign" else [int(step[s, 2]), None] if cls == "foreign_novel" else [None, None]
            rows.append([x, None, None, None, cls] + species[s, j].tolist() + [_frac(species[s, j, 0], species[s, 0, 0]), None, None] + fs + [None, None])
    return rows, species, cd


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


def _resident(eng, sset):
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    eng.get_node_abundances(fetch=False)


def test_profile_seam_rescue(world, capfd, monkeypatch):
    from pantax_amd import _ffi
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng = world
    # a min_cov between the predicted coverages of the table drops its weakest rows: strains that are in the sample and no longer in the table, whose
    # reads no reported strain explains
    _profile(eng, db, root / "wd_all", gaf)
    covs = sorted(float(r[3]) for r in _lines(root / "wd_all" / "strain_abundance.txt")[1:])
    cuts = [int(c) + 1 for c in covs if sum(x < int(c) + 1 for x in covs) >= 1 and sum(x >= int(c) + 1 for x in covs) >= 2]
    assert cuts, covs
    mc = cuts[0]
    plain, wd = root / "wd_plain", root / "wd_rc"
    _profile(eng, db, plain, gaf, min_cov=mc, strain_evidence_file=str(plain / "ev.tsv"))
    _profile(eng, db, wd, gaf, min_cov=mc, strain_evidence_file=str(wd / "ev.tsv"), strain_rescue_file=str(wd / "rc.tsv"))
    for f in ("species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt", "ev.tsv"):   # the option changes no table and no other report
        assert open(wd / f, "rb").read() == open(plain / f, "rb").read(), f
    assert not os.path.exists(plain / "rc.tsv")
    rows = _lines(wd / "rc.tsv")
    assert rows[0] == HEADER
    _resident(eng, sset)
    exp, species, cd = _expected_rows(sset, db, wd, eng, 5)                   # top 0 = the default of 5
    _same_rows(rows[1:], exp)
    n_cand = sum(1 for r in exp if r[4] == "candidate")
    assert n_cand >= 1 and species[:, ref.FOREIGN_RESCUED, 0].sum() > 0 and [r[4] for r in rows[1 + n_cand:]] == list(ref.NAMES) * ((len(rows) - 1 - n_cand) // 9)
    full = open(wd / "rc.tsv", "rb").read()
    # --strain-rescue-top 1
    w1 = root / "wd_rc_top1"
    _profile(eng, db, w1, gaf, min_cov=mc, strain_evidence_file=str(w1 / "ev.tsv"), strain_rescue_file=str(w1 / "rc.tsv"), strain_rescue_top=1)
    _resident(eng, sset)
    exp1, _, _ = _expected_rows(sset, db, w1, eng, 1)
    _same_rows(_lines(w1 / "rc.tsv")[1:], exp1)
    assert all(r[3] == 1 for r in exp1 if r[4] == "candidate")
    # beside the near-miss and the add-one report: one candidate call a group, the same file
    wb = root / "wd_rc_beside"
    _profile(eng, db, wb, gaf, min_cov=mc, strain_rescue_file=str(wb / "rc.tsv"), strain_near_miss_file=str(wb / "nm.tsv"), strain_addin_file=str(wb / "ai.tsv"))
    assert open(wb / "rc.tsv", "rb").read() == full
    # a species-only run writes nothing; the strain-only resume behind it writes the same file
    wr = root / "wd_rc_resume"
    capfd.readouterr()
    _profile(eng, db, wr, gaf, species=True, strain=False, out_binning_file=str(wr / "reads_classification.tsv"), strain_rescue_file=str(wr / "rc_species_only.tsv"))
    assert not os.path.exists(wr / "rc_species_only.tsv") and "no strain step" in capfd.readouterr().err
    _profile(eng, db, wr, gaf, species=False, strain=True, min_cov=mc, strain_rescue_file=str(wr / "rc.tsv"))
    assert open(wr / "rc.tsv", "rb").read() == full
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_rc_cli"
    wc.mkdir()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0", "--min_cov", str(mc),
                        "--strain-rescue", str(wc / "rc.tsv"), "--strain-rescue-top", "5"], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc / "rc.tsv", "rb").read() == full
    # several ranks: refused on every rank with the table's wording, before any collective
    for rank in range(2):
        wn = root / ("wd_rc_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, strain_rescue_file=str(wn / "rc.tsv"))
        assert e.value.code == E_INVALID and "the read rescue report (strain_rescue_file) needs one rank and an unsharded ingest (world_size 2)" in str(e.value)
        assert not os.path.exists(wn / "rc.tsv")
    # a caller compiled against the header before these fields: its struct ends behind strain_mosaic_top, the report reads as off
    real = _ffi.ProfileExt

    class OldExt(real):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.struct_size = 136

    monkeypatch.setattr(_ffi, "ProfileExt", OldExt)
    wold = root / "wd_rc_old"
    _profile(eng, db, wold, gaf, min_cov=mc, strain_fit_file=str(wold / "fit.tsv"), strain_rescue_file=str(wold / "rc.tsv"))
    monkeypatch.setattr(_ffi, "ProfileExt", real)
    assert os.path.exists(wold / "fit.tsv") and not os.path.exists(wold / "rc.tsv")
    assert open(wold / "strain_abundance.txt", "rb").read() == open(wd / "strain_abundance.txt", "rb").read()
