"""GPU tests of the per-strain depth distribution (pantax_hip_strain_depth, --strain-depth).  The expected values come from the row-by-row Python
reading of the contract in tests/depth_ref.py (pinned by tests/test_depth_ref.py on hand-written tables), applied to the bases_per_node that
get_node_abundances hands out -- the parity tests pin those against the oracle.  Everything is an integer: every comparison is np.array_equal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import depth_ref as ref
from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile, seam_world
from tests.hap_stats_cases import pack_reads

pytestmark = pytest.mark.gpu

CHUNK = 2048       # DP_CHUNK of stage_depth.hip: the pass cuts every species' nodes into items of 2048 nodes, taken in slabs of 1024 by 256 threads
E_INVALID, E_STATE = -1, -7


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _coverage(eng, sset):
    """the set resident with a coverage result of the stage kind -> (bases_per_node, node_base_cov); computed once per set"""
    if getattr(eng, "_dp_resident", None) is not sset:
        eng.upload_db(sset.species)
        eng.upload_packed(sset.reads)
        eng.rcls_profile(want_species=False)
        eng.trio_nodes_info()
        bases, cov, _, _ = eng.get_node_abundances()
        sset._dp_cov = (np.array(bases, copy=True), np.array(cov, copy=True))
        eng._dp_resident = sset
    return sset._dp_cov


def _selection(species, pick):
    off, hp = [0], []
    for s, g in enumerate(species):
        hp += list(pick(s, g.n_paths))
        off.append(len(hp))
    return np.array(off, dtype=np.uint64), np.array(hp, dtype=np.uint32)


def _expected(sset, sel):
    bases, cov = sset._dp_cov
    return ref.depth(sset.species, sel[0], sel[1], cov, bases)


def _check(got, exp):
    for a, b in zip(got, exp):
        assert a.dtype == b.dtype == np.uint64 and a.shape == b.shape and np.array_equal(a, b)


def _both_routes(eng, set_opt, sel):
    """the call under the default route, under depth_route=walk, and with the whole pass in two workgroups (depth_grid=2: every workgroup keeps its
    counters across items and flushes where the species or the tile changes): the same numbers"""
    got = eng.strain_depth(*sel)
    for name, value in (("depth_route", "walk"), ("depth_grid", "2")):
        set_opt(eng, name, value)
        try:
            other = eng.strain_depth(*sel)
        finally:
            set_opt(eng, name, None)
        _check(other, got)
    return got


@pytest.fixture(scope="module")
def narrow():
    import synthdata as synth
    return synth.make_set(931, 3, 6, 20000, 80000, present_frac=0.6)


def test_depth_narrow_routes_and_selections(eng, narrow, set_opt):
    """none, one, some (shuffled) and all haplotypes of a species; by the node -> haplotype words and by the walks"""
    sset = narrow
    _coverage(eng, sset)
    assert all(g.n_paths == 6 for g in sset.species)                         # <= 64 haplotypes: the default route is the node -> haplotype words
    V = [g.n_nodes for g in sset.species]
    assert any(v > CHUNK and v % CHUNK and v % 256 for v in V)               # an item border inside a species, a last slab that ends inside a wave
    for pick in (lambda s, H: range(H) if s == 0 else ([] if s == 2 else [4, 0, 2]),
                 lambda s, H: [3] if s == 2 else ([] if s == 0 else range(H)),
                 lambda s, H: []):
        sel = _selection(sset.species, pick)
        exp = _expected(sset, sel)
        _check(_both_routes(eng, set_opt, sel), exp)
    sel = _selection(sset.species, lambda s, H: range(H) if s == 0 else ([] if s == 2 else [4, 0, 2]))
    hap, sp = _expected(sset, sel)
    # the case holds what the kernel can get wrong (computed from the set: a changed generator cannot hollow the test out)
    assert hap[:6, 1].sum() > 0 and hap[6:, 1].sum() > 0 and np.all(hap[:, 1, :, 0].sum(axis=1) < hap[:, 0, :, 0].sum(axis=1))   # private nodes, and shared ones
    assert sp[1, 1].sum() > 0 and np.array_equal(sp[2, 1], sp[2, 0])         # orphans beside a selection; a species without one is all orphan
    assert (sp[:, 0, :, 0] > 0).sum(axis=1).min() >= 4                       # several depths per species: the histogram is not one bin


def _mixed_set(seed, haps, n_reads, genome_len):
    """synthdata.make_set with a haplotype count of its own per species"""
    import synthdata as synth
    rng = np.random.default_rng(seed)
    species, start = [], 1
    for s, h in enumerate(haps):
        g = synth.make_species(rng, str(1000 + s), h, genome_len, start, "GCF_%06d" % (s + 1), present_frac=0.3)
        species.append(g)
        start = g.range_end + 1
    return synth.SyntheticSet(species, synth.make_reads(rng, species, n_reads))


def test_depth_64_and_65_haplotypes(eng, set_opt):
    """the last bit of the one-word route (haplotype 63 of 64), and the first species beyond it (65 haplotypes: compact masks)"""
    sset = _mixed_set(932, [64, 65], 8000, 8000)
    assert [g.n_paths for g in sset.species] == [64, 65]
    _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: [63, 5, 20] if s == 0 else [64, 0, 33])
    exp = _expected(sset, sel)
    assert exp[0][0, 0].sum() > 0 and exp[0][3, 0].sum() > 0 and np.all(exp[1][:, 1, :, 0].sum(axis=1) > 0)
    _check(_both_routes(eng, set_opt, sel), exp)
    full = _selection(sset.species, lambda s, H: range(H))                   # eight full tiles; K = 65: nine tiles, the last with one haplotype in the second word
    _check(_both_routes(eng, set_opt, full), _expected(sset, full))


def test_depth_wide_species_two_mask_words(eng, set_opt):
    """100 of 130 haplotypes in shuffled order: two mask words per node, thirteen tiles; a private node whose only bit lies in the second word"""
    import synthdata as synth
    rng = np.random.default_rng(7)
    sset = synth.make_set(933, 2, 130, 8000, 12000, present_frac=0.6)
    _coverage(eng, sset)
    g = sset.species[0]
    visits = np.zeros((g.n_nodes, 130), dtype=bool)
    for h in range(130):
        visits[g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])], h] = True
    alone = np.nonzero(visits.sum(axis=1) == 1)[0]                           # nodes one haplotype of the db walks alone: private under any selection with it
    assert len(alone) > 0
    h_star = int(np.nonzero(visits[alone[0]])[0][0])
    pick0 = [int(h) for h in rng.permutation(130) if h != h_star][:99]
    pick0.insert(90, h_star)                                                 # ... placed in the second word, in the middle of a tile
    sel = _selection(sset.species, lambda s, H: pick0 if s == 0 else range(0, H, 3))
    exp = _expected(sset, sel)
    assert len(pick0) == 100 and exp[0][90, 1].sum() > 0 and exp[0][:64, 1].sum() > 0   # private nodes whose only bit lies in word 1, and in word 0
    assert exp[1][0, 1].sum() > 0                                            # orphans
    _check(_both_routes(eng, set_opt, sel), exp)


@pytest.fixture(scope="module")
def chunked():
    import synthdata as synth
    return synth.make_set(934, 4, 5, 20000, 30000, present_frac=0.6, single_strain_every=2)


def test_depth_single_strain_chunk_graphs(eng, chunked, set_opt):
    """K = 1: all = private; a single strain that walks every node of its species: = total, nothing orphan"""
    sset = chunked
    assert [g.n_paths for g in sset.species] == [5, 1, 5, 1]
    _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: [0] if H == 1 else ([2] if s == 0 else range(H)))
    got = _both_routes(eng, set_opt, sel)
    _check(got, _expected(sset, sel))
    hap, sp = got
    for s, c in ((0, 0), (1, 1), (3, 7)):                                    # the three species with one selected strain, and its entry
        assert np.array_equal(hap[c, 0], hap[c, 1])
    for s, c in ((1, 1), (3, 7)):
        assert np.array_equal(hap[c, 0], sp[s, 0]) and not sp[s, 1].any() and sp[s, 0].sum() > 0
    assert sp[0, 1].sum() > 0


def _sized_set(seed, sizes, H=3, reads_per_species=60):
    """one species per entry of `sizes` with exactly that many nodes: H walks over random subsets of the nodes (in node order), node lengths 1 .. 40,
    reads that cover two to four consecutive nodes of a walk from end to end"""
    import synthdata as synth
    rng = np.random.default_rng(seed)
    species, lists, start = [], [], 1
    for i, V in enumerate(sizes):
        node_len = rng.integers(1, 41, size=V).astype(np.int64)
        walks = []
        for h in range(H):
            w = np.nonzero(rng.random(V) < 0.6)[0]
            walks.append(w if len(w) else np.array([0]))
        path_off = np.concatenate([[0], np.cumsum([len(w) for w in walks])]).astype(np.uint64)
        names = sorted("GCF_9%03d%03d.1" % (i, h) for h in range(H))
        g = synth.SpeciesGraph(str(3000 + i), node_len, path_off, np.concatenate(walks).astype(np.uint32), names, start, start + V - 1,
                               np.array([node_len[w].sum() for w in walks], dtype=np.int64), np.zeros(H))
        reads = []
        for _ in range(reads_per_species):
            w = walks[int(rng.integers(0, H))]
            k = int(min(len(w), rng.integers(2, 5)))
            a = int(rng.integers(0, len(w) - k + 1))
            nodes = w[a:a + k]
            reads.append((tuple(int(v) + start for v in nodes), 0, int(node_len[nodes].sum())))
        species.append(g)
        lists.append(reads)
        start += V
    return synth.SyntheticSet(species, pack_reads(lists, seed))


def test_depth_node_counts_around_wave_slab_and_chunk(eng, set_opt):
    """species of 1, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 1 nodes: the ends of a wave, of the workgroup's stride and of an item"""
    sizes = [1, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
    sset = _sized_set(935, sizes)
    assert [g.n_nodes for g in sset.species] == sizes
    _coverage(eng, sset)
    for pick in (lambda s, H: [2, 0] if s % 2 else range(H), lambda s, H: [1] if s % 3 else []):
        sel = _selection(sset.species, pick)
        exp = _expected(sset, sel)
        assert np.array_equal(exp[1][:, 0, :, 0].sum(axis=1), np.array(sizes, dtype=np.uint64)) and exp[1][:, 0, 1:].sum() > 0
        _check(_both_routes(eng, set_opt, sel), exp)


def test_depth_above_the_exact_range(eng, set_opt):
    """short nodes under hundreds of reads land in the logarithmic bins; a long node nobody reads stays at depth 0"""
    import synthdata as synth
    #        A   B  C   D     E
    lens = [50, 2, 50, 1000, 3]
    walks = [[0, 1, 2, 3], [0, 2, 4]]
    g = synth.SpeciesGraph("4000", np.array(lens, dtype=np.int64), np.array([0, 4, 7], dtype=np.uint64), np.array(walks[0] + walks[1], dtype=np.uint32),
                           ["GCF_940000.1", "GCF_940001.1"], 1, 5, np.array([1102, 103], dtype=np.int64), np.zeros(2))
    reads = [((1, 2, 3), 0, 102)] * 400 + [((1, 3, 5), 0, 103)] * 350        # A B C whole, 400 times; A C E whole, 350 times
    sset = synth.SyntheticSet([g], pack_reads([reads], 936))
    bases, _ = _coverage(eng, sset)
    d = [int(b) // l for b, l in zip(bases.tolist(), lens)]
    assert d[3] == 0 and d[1] >= 300 and d[4] >= 300 and min(d[0], d[2]) >= 300   # (reads that cover their nodes whole: 750, 400, 750, 0, 350 -- bins 49, 46, 49, 0, 45)
    sel = _selection(sset.species, lambda s, H: [1, 0])
    exp = _expected(sset, sel)
    got = _both_routes(eng, set_opt, sel)
    _check(got, exp)
    hap, sp = got
    assert sp[0, 0, 40:, 0].sum() == 4 and sp[0, 0, :32].sum() == 1 + 1000   # four nodes beyond the exact range (bins >= 40), the long node at depth 0
    assert sp[0, 0, 0].tolist() == [1, 1000] and sp[0, 0, ref.depth_bin(d[1])].tolist() == [1, 2] and sp[0, 0, ref.depth_bin(d[4])].tolist() == [1, 3]
    assert hap[1, 1, 0].tolist() == [1, 1000] and hap[1, 1, 40:, 0].sum() == 1 and hap[0, 1, 40:, 0].sum() == 1 and not sp[0, 1].any()   # private: B and D of walk 0, E of walk 1


def test_depth_sums_to_the_node_evidence(eng, narrow):
    """summed over its bins every histogram gives {n_nodes, len} of the same class of pantax_hip_strain_evidence; without species_out the same hap_out"""
    sset = narrow
    _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: [5, 1, 2] if s == 1 else ([3] if s == 0 else []))
    hap, sp = eng.strain_depth(*sel)
    ev_hap, ev_sp = eng.strain_evidence(*sel)
    assert np.array_equal(hap.sum(axis=2), ev_hap[:, :, :2]) and np.array_equal(sp.sum(axis=2), ev_sp[:, :2, :2])
    only_hap, none = eng.strain_depth(sel[0], sel[1], species=False)         # species_out = NULL
    assert none is None and np.array_equal(only_hap, hap)


def _raw(eng, sel_off, sel_hap, n_species=None, fill=77):
    """the C call as it is: (rc, hap, species); the arrays are pre-filled with `fill`"""
    from pantax_amd import _ffi
    so, sh = np.ascontiguousarray(sel_off, dtype=np.uint64), np.ascontiguousarray(sel_hap, dtype=np.uint32)
    cs = _ffi.EvidenceSet(eng.S if n_species is None else n_species, so.ctypes.data, sh.ctypes.data if len(sh) else None)
    hap = np.full((max(len(sh), 1), 2, 96, 2), fill, dtype=np.uint64)
    sp = np.full((eng.S, 2, 96, 2), fill, dtype=np.uint64)
    rc = eng.lib.pantax_hip_strain_depth(eng.ctx, eng.db, C.byref(cs), _ffi.p(hap), _ffi.p(sp))
    return rc, hap[:len(sh)], sp


def test_depth_state_and_arguments(eng, narrow):
    from pantax_amd._ffi import PantaxHipError
    sset = narrow
    eng._dp_resident = None
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    sel = _selection(sset.species, lambda s, H: [4, 1] if s == 1 else ([H - 1] if s == 0 else []))
    rc, hap, sp = _raw(eng, sel[0], sel[1])
    assert rc == E_STATE and np.all(hap == 77) and np.all(sp == 77)          # no coverage pass yet
    bases, cov, _, _ = eng.get_node_abundances()
    exp = ref.depth(sset.species, sel[0], sel[1], cov, bases)
    rc, hap, sp = _raw(eng, sel[0], sel[1])
    assert rc == 0
    _check((hap, sp), exp)
    # refused arguments: nothing is written
    for args, kw in ((([0, 0, 2, 2], [3, 3]), {}),                           # a haplotype twice within a species
                     (([0, 1, 1, 1], [sset.species[0].n_paths]), {}),        # index = n_paths
                     ((sel[0][:-1], sel[1]), {"n_species": eng.S - 1})):
        rc, hap, sp = _raw(eng, *args, **kw)
        assert rc == E_INVALID and np.all(hap == 77) and np.all(sp == 77)
    # nothing selected: every node of every species is an orphan
    rc, hap, sp = _raw(eng, [0, 0, 0, 0], [])
    assert rc == 0 and len(hap) == 0 and np.array_equal(sp[:, 0], sp[:, 1]) and np.array_equal(sp[:, 0], exp[1][:, 0])
    # a resident step keeps no coverage result of the stage kind and may zero the arena: refused behind it, fine again behind the next stage call
    eng.profile_step(sset.avg_len())
    rc, hap, sp = _raw(eng, sel[0], sel[1])
    assert rc == E_STATE and np.all(hap == 77) and np.all(sp == 77)
    with pytest.raises(PantaxHipError) as e:
        eng.strain_depth(sel[0], sel[1])
    assert e.value.code == E_STATE and "resident step" in str(e.value)
    eng.get_node_abundances(fetch=False)
    _check(eng.strain_depth(sel[0], sel[1]), exp)


# ---- the file seam -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world(tmp_path_factory):
    yield from seam_world(tmp_path_factory, "pantax_dp", 32, 4, 5, 30000, 30000, present_frac=0.4, single_strain_every=4, with_ids=True)   # the small world of test_profile_seam_strain_evidence


OTHER_REPORTS = {"read_strain_file": "rs.tsv", "strain_coverage_file": "ct.tsv", "strain_evidence_file": "ev.tsv", "strain_read_support_file": "sup.tsv"}


def test_profile_seam_strain_depth(world, set_opt):
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng = world
    plain, wd = root / "wd_plain", root / "wd_dp"
    _profile(eng, db, plain, gaf, **{k: str(plain / v) for k, v in OTHER_REPORTS.items()})
    _profile(eng, db, wd, gaf, strain_depth_file=str(wd / "dp.tsv"), **{k: str(wd / v) for k, v in OTHER_REPORTS.items()})
    for f in ["species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt"] + list(OTHER_REPORTS.values()):   # the option changes no table and no other report
        assert open(wd / f, "rb").read() == open(plain / f, "rb").read(), f
    assert not os.path.exists(plain / "dp.tsv")
    rows = _lines(wd / "dp.tsv")
    table = _lines(wd / "strain_abundance.txt")[1:]
    n_str = len(table)
    assert n_str >= 2 and len({tuple(r[:3]) for r in table}) == n_str
    # the stage outputs of the same sample for the table's rows
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    eng.get_node_abundances(fetch=False)
    names = [g.name for g in sset.species]
    genome_hap = {r[0]: r[0].split("_ASM")[0] for r in _lines(db / "genomes_info.txt")[1:]}
    picked = [[] for _ in names]                                             # per species: (haplotype, row of the table), ascending haplotype
    for i, t in enumerate(table):
        s = names.index(t[0])
        picked[s].append((sset.species[s].hap_names.index(genome_hap[t[2]]), i))
    for p in picked:
        p.sort()
    sel_off = np.concatenate([[0], np.cumsum([len(p) for p in picked])]).astype(np.uint64)
    sel_hap = np.array([h for p in picked for h, _ in p], dtype=np.uint32)
    hap, sp = eng.strain_depth(sel_off, sel_hap)
    entry_of_row = {i: int(sel_off[s]) + k for s, p in enumerate(picked) for k, (_, i) in enumerate(p)}
    # the species that went through the strain step, in the run's order: as the node evidence report of the same run lists them
    seq = []
    for r in _lines(wd / "ev.tsv")[1:]:
        if r[3] == "total":
            seq.append(r[0])
    assert len(set(seq)) == len(seq) >= 2 and {t[0] for t in table} <= set(seq)
    strain_rows = rows[1:1 + 2 * n_str]
    assert all(np.float64(strain_rows[2 * i + k][13]) == np.float64(table[i][3]) for i in range(n_str) for k in (0, 1))   # the table's predicted_coverage
    exp = ref.report_rows([(t[0], t[1], t[2], hap[entry_of_row[i], 0], hap[entry_of_row[i], 1], strain_rows[2 * i][13]) for i, t in enumerate(table)],
                          [(x, sp[names.index(x), 0], sp[names.index(x), 1]) for x in seq])
    assert rows == exp
    assert any(r[3] == "private" and int(r[4]) > 0 for r in rows[1:]) and any(r[3] == "orphan" and int(r[5]) > 0 and r[9] != "-" for r in rows[1:])
    # the path that cuts the species into groups: the same file from more than one group
    wg = root / "wd_dp_groups"
    set_opt(eng, "db_path_steps_max", 1)
    try:
        _profile(eng, db, wg, gaf, strain_depth_file=str(wg / "dp.tsv"))
    finally:
        set_opt(eng, "db_path_steps_max", None)
    assert open(wg / "dp.tsv", "rb").read() == open(wd / "dp.tsv", "rb").read()
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_dp_cli"
    wc.mkdir()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0",
                        "--strain-depth", str(wc / "dp.tsv")], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc / "dp.tsv", "rb").read() == open(wd / "dp.tsv", "rb").read()
    # several ranks
    for rank in range(2):
        wn = root / ("wd_dp_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, strain_depth_file=str(wn / "dp.tsv"))
        assert e.value.code == E_INVALID
        assert not os.path.exists(wn / "dp.tsv") and not os.path.exists(wn / "species_abundance.txt")
