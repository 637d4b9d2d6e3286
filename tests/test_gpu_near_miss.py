"""GPU tests of the unreported-strain near misses (pantax_hip_strain_near_miss, --strain-near-miss).  The expected values come from the numpy restatement
of the contract in tests/near_miss_ref.py (pinned by tests/test_near_miss_ref.py on a hand-computed case), applied to the bases_per_node and node_base_cov
that get_node_abundances hands out -- the parity tests pin those against the oracle.  Everything is an integer: every comparison is np.array_equal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile, seam_world
from tests.hap_stats_cases import pack_reads
from tests.near_miss_ref import near_miss, near_miss_rank

pytestmark = pytest.mark.gpu

CHUNK = 1024       # NM_CHUNK of stage_near_miss.hip: the node pass cuts every species' nodes into chunks of 1024 (a wave each), taken in tiles of 256
E_INVALID, E_STATE = -1, -7


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _coverage(eng, sset):
    """the set resident with a coverage result of the stage kind -> (bases_per_node, node_base_cov); computed once per set"""
    if getattr(eng, "_nm_resident", None) is not sset:
        eng.upload_db(sset.species)
        eng.upload_packed(sset.reads)
        eng.rcls_profile(want_species=False)
        eng.trio_nodes_info()
        bases, cov, _, _ = eng.get_node_abundances()
        sset._nm_cov = (np.array(bases, copy=True), np.array(cov, copy=True))
        eng._nm_resident = sset
    return sset._nm_cov


def _sets(species, pick):
    """pick(s, H) -> (reported, candidates) of species s -> (sel_off, sel_hap, cand_off, cand_hap)"""
    so, sh, co, ch = [0], [], [0], []
    for s, g in enumerate(species):
        a, b = pick(s, g.n_paths)
        sh += list(a)
        ch += list(b)
        so.append(len(sh))
        co.append(len(ch))
    return np.array(so, dtype=np.uint64), np.array(sh, dtype=np.uint32), np.array(co, dtype=np.uint64), np.array(ch, dtype=np.uint32)


def _check(got, exp):
    for a, b in zip(got, exp):
        assert a.dtype == b.dtype == np.uint64 and a.shape == b.shape and np.array_equal(a, b)


def _both_routes(eng, set_opt, sets):
    """the call under the default route and under near_miss_route=walk: the same numbers"""
    got = eng.strain_near_miss(*sets)
    set_opt(eng, "near_miss_route", "walk")
    try:
        walk = eng.strain_near_miss(*sets)
    finally:
        set_opt(eng, "near_miss_route", None)
    _check(walk, got)
    return got


def _identities(got, sets, S):
    cand, sp = got
    assert np.all(cand[:, 1] <= cand[:, 0]) and np.all(sp[:, 2] <= sp[:, 1]) and np.all(sp[:, 1] <= sp[:, 0])
    for s in range(S):
        c0, c1 = int(sets[2][s]), int(sets[2][s + 1])
        assert np.array_equal(sp[s, 1], sp[s, 2] + cand[c0:c1, 1].sum(axis=0, dtype=np.uint64))   # claimed = contested + the exclusive sums
        if c1 - c0 == 1:
            assert np.array_equal(cand[c0, 0], cand[c0, 1]) and np.array_equal(cand[c0, 0], sp[s, 1]) and not sp[s, 2].any()


def _cross_checks(eng, got, sets, S):
    """against the node evidence call on the same coverage result: its orphan for the same Sel; novel <= all with Sel = Cand"""
    cand, sp = got
    assert np.array_equal(sp[:, 0], eng.strain_evidence(sets[0], sets[1])[1][:, 1])
    assert np.all(cand[:, 0] <= eng.strain_evidence(sets[2], sets[3])[0][:, 0])


# the selections every shape goes through: (reported, candidates) of a species of H haplotypes
def _selections(seed):
    rng = np.random.default_rng(seed)

    def split(s, H):
        order = [int(h) for h in rng.permutation(H)]
        k = int(rng.integers(0, H))
        return order[:k], order[k:k + int(rng.integers(0, H - k + 1))]
    return {
        "nothing reported, every haplotype a candidate": lambda s, H: ([], range(H)),
        "no candidates": lambda s, H: (range(0, H, 2), []),
        "both empty": lambda s, H: ([], []),
        "all reported but one": lambda s, H: ([h for h in range(H) if h != (s + 1) % H], [(s + 1) % H]),
        "a single candidate": lambda s, H: ([0] if H > 1 else [], [H - 1]),
        "a random split": split,
    }


def _sized_set(seed, sizes, H, density=0.35, reads_per_species=60):
    """one species per entry of `sizes` with exactly that many nodes: H walks over random subsets of the nodes (in node order) -- at this density a fair
    share of the nodes is walked by nobody or by one haplotype --, node lengths 1 .. 40, reads that cover two to four consecutive nodes of a walk"""
    import synthdata as synth
    rng = np.random.default_rng(seed)
    species, lists, start = [], [], 1
    for i, V in enumerate(sizes):
        node_len = rng.integers(1, 41, size=V).astype(np.int64)
        walks = []
        for h in range(H):
            w = np.nonzero(rng.random(V) < density)[0]
            walks.append(w if len(w) else np.array([0]))
        path_off = np.concatenate([[0], np.cumsum([len(w) for w in walks])]).astype(np.uint64)
        names = sorted("GCF_8%03d%03d.1" % (i, h) for h in range(H))
        g = synth.SpeciesGraph(str(4000 + i), node_len, path_off, np.concatenate(walks).astype(np.uint32), names, start, start + V - 1,
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


@pytest.fixture(scope="module")
def sized():
    # a single node; one node short of a chunk, a chunk, one node more (a second chunk of one node); two chunks and a tile's end inside a wave; a few nodes:
    # the chunk list crosses a species border at every one of them
    return _sized_set(941, [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 300, 5], H=6)


@pytest.mark.parametrize("which", list(_selections(0)))
def test_near_miss_chunk_shapes_and_selections(eng, sized, set_opt, which):
    sset = sized
    assert [g.n_nodes for g in sset.species] == [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 300, 5]
    bases, cov = _coverage(eng, sset)
    sets = _sets(sset.species, _selections(942)[which])
    exp = near_miss(sset.species, *sets, cov, bases)
    assert exp[1][:, 0, 0].sum() > 0 and (which != "nothing reported, every haplotype a candidate" or
                                          (exp[1][:, 0, 0].tolist() == [g.n_nodes for g in sset.species] and exp[0][:, 1, 3].sum() > 0 and exp[1][:, 2, 3].sum() > 0))
    got = _both_routes(eng, set_opt, sets)
    _check(got, exp)
    _identities(got, sets, len(sset.species))
    _cross_checks(eng, got, sets, len(sset.species))


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


def test_near_miss_64_and_65_haplotypes(eng, set_opt):
    """the last bit of the one-word route is a candidate's (haplotype 63 of 64); 65 haplotypes: the walk route by itself, two words when every haplotype is listed"""
    sset = _mixed_set(943, [64, 65], 8000, 8000)
    assert [g.n_paths for g in sset.species] == [64, 65]
    bases, cov = _coverage(eng, sset)
    for pick in (lambda s, H: ([5, 20, 40], [63, 0, 33] if s == 0 else [64, 1, 30]),
                 lambda s, H: ([7], [h for h in range(H) if h != 7]),                # every other bit of the word a candidate; 65: Sel ends at bit 1, the candidates reach word 1
                 lambda s, H: ([], list(range(H - 1, -1, -1)))):                     # all 64 bits; all 65 in two words, in descending order
        sets = _sets(sset.species, pick)
        exp = near_miss(sset.species, *sets, cov, bases)
        assert exp[0][0, 0, 0] > 0 and np.all(exp[1][:, 1, 0] > 0)                  # the candidate on bit 63 / 64 (or the first listed) walks orphan nodes
        got = _both_routes(eng, set_opt, sets)
        _check(got, exp)
        _identities(got, sets, 2)
        _cross_checks(eng, got, sets, 2)


def test_near_miss_wide_species_three_candidate_words(eng, set_opt):
    """200 haplotypes: 70 reported in shuffled order (Sel ends at bit 6 of word 1), the other 130 candidates on the words 1, 2 and 3 -- counted in one pass
    over the nodes, and, with near_miss_words = 1 and 2, in tiled passes"""
    import synthdata as synth
    rng = np.random.default_rng(11)
    sset = synth.make_set(944, 2, 200, 6000, 40000, present_frac=0.15)
    bases, cov = _coverage(eng, sset)
    order = [int(h) for h in rng.permutation(200)]
    sets = _sets(sset.species, lambda s, H: (order[:70], order[70:]) if s == 0 else (order[:3], order[100:170]))
    exp = near_miss(sset.species, *sets, cov, bases)
    cand, sp = exp
    assert all(g.n_nodes > 2 * CHUNK for g in sset.species)                         # several chunks add into the counters of every word
    assert sp[0, 2, 0] > 0 and sp[1, 2, 0] > 0 and sp[1, 1, 0] < sp[1, 0, 0]        # contested nodes; species 1 (73 of its 200 haplotypes listed) has orphans nobody claims
    for a, b in ((0, 58), (58, 122), (122, 130)):                                    # candidates of each of the three words walk orphan nodes; some alone
        assert cand[a:b, 0, 0].sum() > 0
    assert cand[:130, 1, 0].sum() > 0
    got = _both_routes(eng, set_opt, sets)
    _check(got, exp)
    _identities(got, sets, 2)
    _cross_checks(eng, got, sets, 2)
    for words in (1, 2):
        set_opt(eng, "near_miss_words", words)
        try:
            _check(eng.strain_near_miss(*sets), exp)
        finally:
            set_opt(eng, "near_miss_words", None)


def _raw(eng, sets, n_species=None, fill=77):
    """the C call as it is: (rc, cand, species); the arrays are pre-filled with `fill`"""
    from pantax_amd import _ffi
    so, sh, co, ch = (np.ascontiguousarray(a, dtype=t) for a, t in zip(sets, (np.uint64, np.uint32, np.uint64, np.uint32)))
    cs = _ffi.NearMissSet(eng.S if n_species is None else n_species, so.ctypes.data, sh.ctypes.data if len(sh) else None, co.ctypes.data,
                          ch.ctypes.data if len(ch) else None)
    cand = np.full((max(len(ch), 1), 2, 4), fill, dtype=np.uint64)
    sp = np.full((eng.S, 3, 4), fill, dtype=np.uint64)
    rc = eng.lib.pantax_hip_strain_near_miss(eng.ctx, eng.db, C.byref(cs), _ffi.p(cand), _ffi.p(sp))
    return rc, cand[:len(ch)], sp


def test_near_miss_state_and_arguments(eng):
    import synthdata as synth
    from pantax_amd._ffi import PantaxHipError
    sset = synth.make_set(921, 3, 6, 20000, 30000, present_frac=0.6)
    eng._nm_resident = None
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    sets = _sets(sset.species, lambda s, H: ([4, 1], [0, 5, 2]) if s == 1 else (([H - 1], [3]) if s == 0 else ([], [])))
    assert _raw(eng, sets)[0] == E_STATE                                     # no coverage pass yet
    bases, cov, _, _ = eng.get_node_abundances()
    exp = near_miss(sset.species, *sets, cov, bases)
    rc, cand, sp = _raw(eng, sets)
    assert rc == 0
    _check((cand, sp), exp)
    assert exp[0][:, 0, 3].sum() > 0
    # refused arguments: nothing is written
    nh = sset.species[0].n_paths
    for bad, kw in ((([0, 0, 2, 2], [3, 3], [0, 0, 0, 0], []), {}),                  # a haplotype twice within Sel
                    (([0, 0, 0, 0], [], [0, 0, 2, 2], [3, 3]), {}),                  # ... within Cand
                    (([0, 1, 1, 1], [nh], [0, 0, 0, 0], []), {}),                    # a reported index = n_paths
                    (([0, 0, 0, 0], [], [0, 1, 1, 1], [nh]), {}),                    # a candidate index = n_paths
                    (([0, 1, 2, 2], [2, 4], [0, 1, 3, 3], [0, 1, 4]), {}),           # haplotype 4 of species 1 in both sets
                    ((sets[0][:-1], sets[1], sets[2][:-1], sets[3]), {"n_species": eng.S - 1})):
        rc, cand, sp = _raw(eng, bad, **kw)
        assert rc == E_INVALID and np.all(cand == 77) and np.all(sp == 77), bad
    # a resident step keeps no node_base_cov and may zero the arena: refused behind it, fine again behind the next stage call
    eng.profile_step(sset.avg_len())
    with pytest.raises(PantaxHipError) as e:
        eng.strain_near_miss(*sets)
    assert e.value.code == E_STATE and "resident step" in str(e.value)
    eng.get_node_abundances(fetch=False)
    _check(eng.strain_near_miss(*sets), exp)


# ---- the file seam -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world(tmp_path_factory):
    yield from seam_world(tmp_path_factory, "pantax_nm", 32, 4, 5, 30000, 30000, present_frac=0.4, single_strain_every=4, with_ids=True)   # the small world of test_profile_seam_strain_evidence


HEADER = ["species_taxid", "strain_taxid", "genome_ID", "rank", "class", "n_nodes", "len", "covered", "bases", "depth", "breadth", "share", "stage",
          "unique_trio_nodes_fraction", "frequencies_mean", "first_sol", "second_sol"]
OTHER_REPORTS = {"strain_evidence_file": "ev.tsv", "strain_depth_file": "dp.tsv"}


def _ratio(a, b):
    return np.float64(a) / np.float64(b)


def _expected_rows(sset, db, wd, eng, top):
    """the report from the stage calls and the run's tables: Sel = the rows of strain_abundance.txt, Cand = every other haplotype (the world's species are
    narrow), the metric cells and the stage from ori_strain_abundance.txt (the unrounded metrics of every haplotype of a reported species)"""
    table = _lines(wd / "strain_abundance.txt")[1:]
    ori = {(r[0], r[2]): r for r in _lines(wd / "ori_strain_abundance.txt")[1:]}
    names = [g.name for g in sset.species]
    genomes = _lines(db / "genomes_info.txt")[1:]
    genome_of = {}
    for r in genomes:
        genome_of.setdefault(r[0].split("_ASM")[0], r)                       # the first row of every haplotype
    col = {c: i for i, c in enumerate(_lines(db / "genomes_info.txt")[0])}
    hap_of_genome = {r[0]: r[0].split("_ASM")[0] for r in genomes}
    reported = [set() for _ in names]
    for t in table:
        reported[names.index(t[0])].add(sset.species[names.index(t[0])].hap_names.index(hap_of_genome[t[2]]))
    sets = _sets(sset.species, lambda s, H: (sorted(reported[s]), [h for h in range(H) if h not in reported[s]]))
    cand, sp = eng.strain_near_miss(*sets)
    seq = [r[0] for r in _lines(wd / "ev.tsv")[1:] if r[3] == "total"]       # the species that went through the strain step, in the run's order
    assert len(set(seq)) == len(seq) >= 2 and {t[0] for t in table} <= set(seq)
    printed = []                                                             # (species, haplotype, candidate entry, rank)
    for x in seq:
        s = names.index(x)
        c0, c1 = int(sets[2][s]), int(sets[2][s + 1])
        for k, c in enumerate(near_miss_rank(sets[3][c0:c1], cand[c0:c1], top)):
            printed.append((s, int(sets[3][c0 + c]), c0 + c, k + 1))
    p_sets = _sets(sset.species, lambda s, H: ([h for q, h, _, _ in printed if q == s], []))
    ev_all = eng.strain_evidence(p_sets[0], p_sets[1])[0][:, 0]
    entry = {(s, h): i for i, (s, h) in enumerate((s, int(h)) for s in range(len(names)) for h in p_sets[1][int(p_sets[0][s]):int(p_sets[0][s + 1])])}

    def cells(q, share_of):
        out = [str(int(x)) for x in q]
        out += [repr_f(_ratio(q[3], q[1])), repr_f(_ratio(q[2], q[1]))] if int(q[1]) else ["-", "-"]
        out.append(repr_f(_ratio(q[3], share_of)) if share_of is not None and int(share_of) else "-")
        return out
    rows, floats = [], []
    for s, h, c, rank in printed:
        g = genome_of.get(sset.species[s].hap_names[h])
        o = ori.get((names[s], g[0] if g else ""))
        assert o is not None, "a printed candidate of a species without rows in ori_strain_abundance.txt"
        stage = "first_filter" if o[8] == "" else ("second_filter" if o[3] == "" else "table_filter")
        metrics = [o[6] or "-", o[7] or "-", o[8] or "-", o[3] or "-"]
        head = [names[s], g[col["strain_taxid"]] if g else "", g[0] if g else "", str(rank)]
        for cls, q, share_of in (("novel", cand[c, 0], sp[s, 0, 3]), ("exclusive", cand[c, 1], sp[s, 0, 3]), ("all", ev_all[entry[(s, h)]], None)):
            rows.append(head + [cls] + cells(q, share_of) + [stage] + metrics)
    for x in seq:
        s = names.index(x)
        for k, cls in enumerate(("orphan", "claimed", "contested")):
            rows.append([x, "-", "-", "-", cls] + cells(sp[s, k], sp[s, 0, 3]) + ["-"] * 5)
    return rows, printed, sp


def repr_f(x):
    """a float cell is compared as the float it parses to"""
    return np.float64(x)


def _same_rows(got, exp):
    assert len(got) == len(exp)
    for a, b in zip(got, exp):
        assert len(a) == len(b) == len(HEADER)
        for x, y in zip(a, b):
            if isinstance(y, np.float64):
                assert np.float64(x) == y, (a, b)
            else:
                assert x == y, (a, b)


def test_profile_seam_strain_near_miss(world, set_opt, capfd):
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng = world
    # the world's reads come from its present strains and the strain step finds them: nothing unreported has coverage.  A min_cov between the predicted
    # coverages of the table drops its weakest rows at the a15 filter -- strains that are in the sample and no longer in the table, the case the report is for
    _profile(eng, db, root / "wd_all", gaf)
    covs = sorted(float(r[3]) for r in _lines(root / "wd_all" / "strain_abundance.txt")[1:])
    cuts = [int(c) + 1 for c in covs if sum(x < int(c) + 1 for x in covs) >= 1 and sum(x >= int(c) + 1 for x in covs) >= 2]
    assert cuts, covs
    mc = cuts[0]
    plain, wd = root / "wd_plain", root / "wd_nm"
    _profile(eng, db, plain, gaf, min_cov=mc, **{k: str(plain / v) for k, v in OTHER_REPORTS.items()})
    _profile(eng, db, wd, gaf, min_cov=mc, strain_near_miss_file=str(wd / "nm.tsv"), **{k: str(wd / v) for k, v in OTHER_REPORTS.items()})
    assert len(_lines(wd / "strain_abundance.txt")) < len(_lines(root / "wd_all" / "strain_abundance.txt"))
    for f in ["species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt"] + list(OTHER_REPORTS.values()):   # the option changes no table and no other report
        assert open(wd / f, "rb").read() == open(plain / f, "rb").read(), f
    assert not os.path.exists(plain / "nm.tsv")
    rows = _lines(wd / "nm.tsv")
    assert rows[0] == HEADER
    # the stage outputs of the same sample
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    eng.get_node_abundances(fetch=False)
    exp, printed, sp = _expected_rows(sset, db, wd, eng, 5)                   # top 0 = the default of 5
    _same_rows(rows[1:], exp)
    n_cand = 3 * len(printed)
    assert len(printed) >= 1 and any(r[12] == "table_filter" and r[4] == "novel" and int(r[8]) > 0 for r in rows[1:]) and [r[4] for r in rows[1:1 + n_cand]] == ["novel", "exclusive", "all"] * len(printed)   # candidate rows first, three classes each ...
    assert [r[4] for r in rows[1 + n_cand:]] == ["orphan", "claimed", "contested"] * ((len(rows) - 1 - n_cand) // 3)   # ... then the species
    assert all(r[11] == "-" for r in rows[1:] if r[4] == "all") and all(r[3] == "-" and r[12] == "-" for r in rows[1 + n_cand:])
    assert {r[12] for r in rows[1:1 + n_cand]} <= {"first_filter", "second_filter", "table_filter"}
    assert all((r[15] == "-") == (r[12] == "first_filter") and (r[16] == "-") == (r[12] != "table_filter") for r in rows[1:1 + n_cand])
    assert sp[:, 0, 3].sum() > 0 and any(r[4] == "novel" and r[11] != "-" for r in rows[1:])
    # the cut: top 1 keeps the first candidate of every species, a large top keeps every candidate with novel bases
    for top, name in ((1, "nm1.tsv"), (1000, "nm_all.tsv")):
        wt = root / ("wd_nm_top%d" % top)
        _profile(eng, db, wt, gaf, min_cov=mc, strain_near_miss_file=str(wt / name), strain_near_miss_top=top, strain_evidence_file=str(wt / "ev.tsv"))
        eng.upload_db(sset.species)
        eng.upload_packed(sset.reads)
        eng.rcls_profile(want_species=False)
        eng.trio_nodes_info()
        eng.get_node_abundances(fetch=False)
        exp_t, printed_t, _ = _expected_rows(sset, db, wt, eng, top)
        _same_rows(_lines(wt / name)[1:], exp_t)
        assert all(rank == 1 for _, _, _, rank in printed_t) if top == 1 else len(printed_t) >= len(printed)
    # the path that cuts the species into groups: the same file from more than one group
    wg = root / "wd_nm_groups"
    set_opt(eng, "db_path_steps_max", 1)
    try:
        _profile(eng, db, wg, gaf, min_cov=mc, strain_near_miss_file=str(wg / "nm.tsv"))
    finally:
        set_opt(eng, "db_path_steps_max", None)
    assert open(wg / "nm.tsv", "rb").read() == open(wd / "nm.tsv", "rb").read()
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_nm_cli"
    wc.mkdir()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0", "--min_cov", str(mc),
                        "--strain-near-miss", str(wc / "nm.tsv"), "--strain-near-miss-top", "5"], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc / "nm.tsv", "rb").read() == open(wd / "nm.tsv", "rb").read()
    # the strain-only resume writes the same file; a run without a strain step writes nothing and says so
    wr = root / "wd_nm_resume"
    _profile(eng, db, wr, gaf, species=True, strain=False, out_binning_file=str(wr / "reads_classification.tsv"), strain_near_miss_file=str(wr / "nm_species.tsv"))
    assert not os.path.exists(wr / "nm_species.tsv")
    _profile(eng, db, wr, gaf, species=False, strain=True, min_cov=mc, strain_near_miss_file=str(wr / "nm.tsv"))
    assert open(wr / "nm.tsv", "rb").read() == open(wd / "nm.tsv", "rb").read()
    capfd.readouterr()
    _profile(eng, db, wr, gaf, species=True, strain=True, strain_near_miss_file=str(wr / "nm_again.tsv"))
    assert not os.path.exists(wr / "nm_again.tsv") and "no strain step" in capfd.readouterr().err
    # a negative top; several ranks
    wn = root / "wd_nm_negative"
    with pytest.raises(PantaxHipError) as e:
        _profile(eng, db, wn, gaf, strain_near_miss_file=str(wn / "nm.tsv"), strain_near_miss_top=-1)
    assert e.value.code == E_INVALID and not os.path.exists(wn / "nm.tsv") and not os.path.exists(wn / "species_abundance.txt")
    for rank in range(2):
        wn = root / ("wd_nm_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, strain_near_miss_file=str(wn / "nm.tsv"))
        assert e.value.code == E_INVALID
        assert not os.path.exists(wn / "nm.tsv") and not os.path.exists(wn / "species_abundance.txt")
