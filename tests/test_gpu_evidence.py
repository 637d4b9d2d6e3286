"""GPU tests of the per-strain node evidence (pantax_hip_strain_evidence, --strain-evidence).  The expected values come from the numpy restatement of
the contract in tests/evidence_ref.py (pinned by tests/test_evidence_ref.py on a hand-computed case), applied to the bases_per_node and node_base_cov
that get_node_abundances hands out -- the parity tests pin those against the oracle.  Everything is an integer: every comparison is np.array_equal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile, seam_world
from tests.evidence_ref import evidence

pytestmark = pytest.mark.gpu

CHUNK = 1024       # the node pass cuts every species' nodes into chunks of 1024 (a wave each), taken in tiles of 256, 64 lanes wide
E_INVALID, E_STATE = -1, -7


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _coverage(eng, sset):
    """the set resident with a coverage result of the stage kind -> (bases_per_node, node_base_cov); computed once per set"""
    if getattr(eng, "_ev_resident", None) is not sset:
        eng.upload_db(sset.species)
        eng.upload_packed(sset.reads)
        eng.rcls_profile(want_species=False)
        eng.trio_nodes_info()
        bases, cov, _, _ = eng.get_node_abundances()
        sset._ev_cov = (np.array(bases, copy=True), np.array(cov, copy=True))
        eng._ev_resident = sset
    return sset._ev_cov


def _selection(species, pick):
    off, hp = [0], []
    for s, g in enumerate(species):
        hp += list(pick(s, g.n_paths))
        off.append(len(hp))
    return np.array(off, dtype=np.uint64), np.array(hp, dtype=np.uint32)


def _check(got, exp):
    for a, b in zip(got, exp):
        assert a.dtype == b.dtype == np.uint64 and a.shape == b.shape and np.array_equal(a, b)


def _both_routes(eng, set_opt, sel):
    """the call under the default route and under evidence_route=walk: the same numbers"""
    got = eng.strain_evidence(*sel)
    set_opt(eng, "evidence_route", "walk")
    try:
        walk = eng.strain_evidence(*sel)
    finally:
        set_opt(eng, "evidence_route", None)
    _check(walk, got)
    return got


@pytest.fixture(scope="module")
def narrow():
    import synthdata as synth
    return synth.make_set(921, 3, 6, 20000, 30000, present_frac=0.6)


def test_evidence_narrow_routes_and_selections(eng, narrow, set_opt):
    """all haplotypes of one species, a shuffled three of the next, none of the last; by the node -> haplotype words and by the walks"""
    sset = narrow
    bases, cov = _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: range(H) if s == 0 else ([] if s == 2 else [4, 0, 2]))
    exp = evidence(sset.species, sel[0], sel[1], cov, bases)
    # the case holds what the kernel can get wrong (computed from the set: a changed generator cannot hollow the test out)
    V = [g.n_nodes for g in sset.species]
    assert all(g.n_paths == 6 for g in sset.species)                         # <= 64 haplotypes: the default route is the node -> haplotype words
    assert any(v % 64 and v % CHUNK for v in V)                              # a last tile that ends inside a wave
    assert any(v > CHUNK for v in V)                                         # a chunk border inside a species
    hap, sp = exp
    assert hap[:6, 1, 0].sum() > 0 and hap[6:, 1, 0].sum() > 0 and np.all(hap[:, 1, 0] < hap[:, 0, 0])   # private nodes in both species, shared ones for every strain
    assert np.all(sp[:2, 2, 0] > 0) and np.all(sp[:2, 2, 0] < sp[:2, 0, 0])  # core nodes, and others
    assert sp[1, 1, 0] > 0 and np.array_equal(sp[2, 1], sp[2, 0])            # orphans beside a selection; a species without one is all orphan
    assert hap[:, :, 2].sum() > 0 and hap[:, :, 3].sum() > 0
    _check(_both_routes(eng, set_opt, sel), exp)


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


def test_evidence_64_and_65_haplotypes(eng, set_opt):
    """the last bit of the one-word route (haplotype 63 of 64), and the first species beyond it (65 haplotypes: compact masks, one word)"""
    sset = _mixed_set(922, [64, 65], 8000, 8000)
    assert [g.n_paths for g in sset.species] == [64, 65]
    bases, cov = _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: [63, 5, 20] if s == 0 else [64, 0, 33])
    exp = evidence(sset.species, sel[0], sel[1], cov, bases)
    assert exp[0][0, 0, 0] > 0 and exp[0][3, 0, 0] > 0 and np.all(exp[1][:, 1, 0] > 0)
    _check(_both_routes(eng, set_opt, sel), exp)
    full = _selection(sset.species, lambda s, H: range(H))                   # every bit of the word; K = 65: two words, one candidate in the second
    _check(_both_routes(eng, set_opt, full), evidence(sset.species, full[0], full[1], cov, bases))


def test_evidence_wide_species(eng, set_opt):
    """80 of 100 haplotypes in shuffled order: two mask words per node, private and core decided over both"""
    import synthdata as synth
    rng = np.random.default_rng(7)
    sset = synth.make_set(923, 2, 100, 8000, 12000, present_frac=0.6)
    bases, cov = _coverage(eng, sset)
    g = sset.species[0]
    visits = np.zeros((g.n_nodes, 100), dtype=bool)
    for h in range(100):
        visits[g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])], h] = True
    alone = np.nonzero(visits.sum(axis=1) == 1)[0]                           # nodes one haplotype of the db walks alone: private under any selection with it
    assert len(alone) > 0
    h_star = int(np.nonzero(visits[alone[0]])[0][0])
    pick0 = [int(h) for h in rng.permutation(100) if h != h_star][:79]
    pick0.insert(70, h_star)                                                 # ... placed in the second word
    sel = _selection(sset.species, lambda s, H: pick0 if s == 0 else range(0, H, 3))
    exp = evidence(sset.species, sel[0], sel[1], cov, bases)
    assert len(pick0) == 80 and exp[0][70, 1, 0] > 0 and exp[0][:64, 1, 0].sum() > 0   # private nodes whose only bit lies in word 1, and in word 0
    assert exp[1][0, 2, 0] > 0 and exp[1][0, 1, 0] > 0                       # core over both words; orphans
    _check(_both_routes(eng, set_opt, sel), exp)


@pytest.fixture(scope="module")
def chunked():
    import synthdata as synth
    return synth.make_set(924, 4, 5, 20000, 30000, present_frac=0.6, single_strain_every=2)


def test_evidence_single_strain_chunk_graphs(eng, chunked, set_opt):
    """K = 1: all = private = core; a single strain that walks every node of its species: = total, nothing orphan"""
    sset = chunked
    assert [g.n_paths for g in sset.species] == [5, 1, 5, 1]
    bases, cov = _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: [0] if H == 1 else ([2] if s == 0 else range(H)))
    got = _both_routes(eng, set_opt, sel)
    _check(got, evidence(sset.species, sel[0], sel[1], cov, bases))
    hap, sp = got
    for s, c in ((0, 0), (1, 1), (3, 7)):                                    # the three species with one selected strain, and its entry
        assert int(sel[0][s + 1] - sel[0][s]) == 1
        assert np.array_equal(hap[c, 0], hap[c, 1]) and np.array_equal(hap[c, 0], sp[s, 2])
    for s, c in ((1, 1), (3, 7)):
        g = sset.species[s]
        assert len(np.unique(g.path_nodes)) == g.n_nodes                     # the strain walks every node
        assert np.array_equal(hap[c, 0], sp[s, 0]) and not sp[s, 1].any() and sp[s, 0, 3] > 0
    assert sp[0, 1, 0] > 0 and sp[0, 2, 0] < sp[0, 0, 0]                     # one strain of five leaves orphans


def test_evidence_long_reads(eng):
    """long reads on 300-kb genomes: more aligned bases than the genome is long, exact in u64"""
    import synthdata as synth
    sset = synth.make_set(925, 2, 6, 400, 300000, long_reads=True, present_frac=0.6)
    bases, cov = _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: [1, 4, 2] if s == 0 else range(H))
    got = eng.strain_evidence(*sel)
    _check(got, evidence(sset.species, sel[0], sel[1], cov, bases))
    assert all(g.n_nodes > 8 * CHUNK for g in sset.species)                  # many chunks add into the same counters
    assert np.any(got[0][:, 0, 3] > got[0][:, 0, 1]) and np.all(got[1][:, 0, 3] > got[1][:, 0, 1])


def test_evidence_ties_to_coverage_track(eng, narrow):
    """for a haplotype whose walk repeats no node, `all` is the sum of its windows of the coverage track"""
    sset = narrow
    _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: [5, 1] if s == 1 else ([3] if s == 0 else []))
    hap, _ = eng.strain_evidence(*sel)
    win_off, n, ln, cv, bs = eng.strain_cov_track(sel[0], sel[1], 10 ** 9)
    assert np.array_equal(np.diff(win_off.astype(np.int64)), np.ones(3, dtype=np.int64))   # one window per strain
    checked = 0
    for c, (s, h) in enumerate(((0, 3), (1, 5), (1, 1))):
        g = sset.species[s]
        walk = g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])]
        if len(np.unique(walk)) != len(walk):
            continue                                                         # (the track counts visits, the evidence nodes)
        assert hap[c, 0].tolist() == [int(n[c]), int(ln[c]), int(cv[c]), int(bs[c])]
        checked += 1
    assert checked > 0, "no selected walk without a repeated node"


def _raw(eng, sel_off, sel_hap, n_species=None, fill=77):
    """the C call as it is: (rc, hap, species); the arrays are pre-filled with `fill`"""
    from pantax_amd import _ffi
    so, sh = np.ascontiguousarray(sel_off, dtype=np.uint64), np.ascontiguousarray(sel_hap, dtype=np.uint32)
    cs = _ffi.EvidenceSet(eng.S if n_species is None else n_species, so.ctypes.data, sh.ctypes.data if len(sh) else None)
    hap = np.full((max(len(sh), 1), 2, 4), fill, dtype=np.uint64)
    sp = np.full((eng.S, 3, 4), fill, dtype=np.uint64)
    rc = eng.lib.pantax_hip_strain_evidence(eng.ctx, eng.db, C.byref(cs), _ffi.p(hap), _ffi.p(sp))
    return rc, hap[:len(sh)], sp


def test_evidence_state_and_arguments(eng, narrow):
    from pantax_amd._ffi import PantaxHipError
    sset = narrow
    eng._ev_resident = None
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    sel = _selection(sset.species, lambda s, H: [4, 1] if s == 1 else ([H - 1] if s == 0 else []))
    assert _raw(eng, sel[0], sel[1])[0] == E_STATE                           # no coverage pass yet
    bases, cov, _, _ = eng.get_node_abundances()
    exp = evidence(sset.species, sel[0], sel[1], cov, bases)
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
    assert rc == 0 and len(hap) == 0 and np.array_equal(sp[:, 0], sp[:, 1]) and not sp[:, 2].any()
    assert sp[:, 0, 0].tolist() == [g.n_nodes for g in sset.species] and np.array_equal(sp[:, 0], exp[1][:, 0])
    # a resident step keeps no node_base_cov and may zero the arena: refused behind it, fine again behind the next stage call
    eng.profile_step(sset.avg_len())
    with pytest.raises(PantaxHipError) as e:
        eng.strain_evidence(sel[0], sel[1])
    assert e.value.code == E_STATE and "resident step" in str(e.value)
    eng.get_node_abundances(fetch=False)
    _check(eng.strain_evidence(sel[0], sel[1]), exp)


# ---- the file seam -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world(tmp_path_factory):
    yield from seam_world(tmp_path_factory, "pantax_ev", 32, 4, 5, 30000, 30000, present_frac=0.4, single_strain_every=4, with_ids=True)


HEADER = ["species_taxid", "strain_taxid", "genome_ID", "class", "n_nodes", "len", "covered", "bases", "depth", "breadth", "predicted_coverage"]


def test_profile_seam_strain_evidence(world, set_opt, capfd):
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng = world
    _profile(eng, db, root / "wd_plain", gaf)
    wd = root / "wd_ev"
    _profile(eng, db, wd, gaf, strain_evidence_file=str(wd / "ev.tsv"))
    for f in ("species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt"):   # the option changes none of the tables
        assert open(wd / f, "rb").read() == open(root / "wd_plain" / f, "rb").read()
    assert not os.path.exists(root / "wd_plain" / "ev.tsv")
    rows = _lines(wd / "ev.tsv")
    assert rows[0] == HEADER and all(len(r) == len(HEADER) for r in rows)
    rows = rows[1:]
    table = _lines(wd / "strain_abundance.txt")[1:]
    n_str = len(table)
    assert n_str >= 2 and len({tuple(r[:3]) for r in table}) == n_str
    # strain rows first: all, then private, per row of the table in its order, with the table's predicted_coverage
    assert [(tuple(r[:3]), r[3]) for r in rows[:2 * n_str]] == [(tuple(t[:3]), cls) for t in table for cls in ("all", "private")]
    assert all(np.float64(rows[2 * i + k][10]) == np.float64(table[i][3]) for i in range(n_str) for k in (0, 1))
    sp_rows = rows[2 * n_str:]
    assert all(r[1] == "-" and r[2] == "-" and r[3] in ("total", "orphan", "core") for r in sp_rows)
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
    hap, sp = eng.strain_evidence(sel_off, sel_hap)
    entry_of_row = {i: int(sel_off[s]) + k for s, p in enumerate(picked) for k, (_, i) in enumerate(p)}
    ints = lambda r: [int(x) for x in r[4:8]]
    for i in range(n_str):
        assert ints(rows[2 * i]) == hap[entry_of_row[i], 0].tolist() and ints(rows[2 * i + 1]) == hap[entry_of_row[i], 1].tolist()
    # species rows: every species that went through the strain step, in the run's order; core only where the species has rows
    seq = []
    for r in sp_rows:
        if not seq or seq[-1] != r[0]:
            seq.append(r[0])
    idx = [names.index(x) for x in seq]
    sp_table = [r[0] for r in _lines(wd / "species_abundance.txt")[1:]]          # the run takes the selected species in the order of the species table
    assert len(set(seq)) == len(seq) >= 2 and seq == [x for x in sp_table if x in set(seq)] and {t[0] for t in table} <= set(seq)
    at = 0
    for s in idx:
        classes = ["total", "orphan"] + (["core"] if picked[s] else [])
        mine = sp_rows[at:at + len(classes)]
        at += len(classes)
        assert [r[3] for r in mine] == classes and all(r[0] == names[s] for r in mine)
        for r, k in zip(mine, range(3)):
            assert ints(r) == sp[s, k].tolist()
        assert mine[0][10] == "-" and mine[1][10] == "-"
        if picked[s]:
            pc = np.float64(0.0)
            for _, i in picked[s]:                                           # ascending haplotype index
                pc += np.float64(table[i][3])
            assert np.float64(mine[2][10]) == pc
    assert at == len(sp_rows)
    for r in rows:                                                           # the two ratios parse back bit for bit; "-" without bases of length
        if int(r[5]):
            assert np.float64(r[8]) == np.float64(int(r[7])) / np.float64(int(r[5])) and np.float64(r[9]) == np.float64(int(r[6])) / np.float64(int(r[5]))
        else:
            assert r[8] == "-" and r[9] == "-"
    assert any(r[3] == "private" and int(r[4]) > 0 for r in rows) and any(r[3] == "core" and int(r[7]) > 0 for r in rows)
    # the path that cuts the species into groups: the same file from more than one group
    wg = root / "wd_ev_groups"
    set_opt(eng, "db_path_steps_max", 1)
    try:
        _profile(eng, db, wg, gaf, strain_evidence_file=str(wg / "ev.tsv"))
    finally:
        set_opt(eng, "db_path_steps_max", None)
    assert open(wg / "ev.tsv", "rb").read() == open(wd / "ev.tsv", "rb").read()
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_ev_cli"
    wc.mkdir()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0",
                        "--strain-evidence", str(wc / "ev.tsv")], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc / "ev.tsv", "rb").read() == open(wd / "ev.tsv", "rb").read()
    # the strain-only resume writes the same file; a run without a strain step writes nothing and says so
    wr = root / "wd_ev_resume"
    _profile(eng, db, wr, gaf, species=True, strain=False, out_binning_file=str(wr / "reads_classification.tsv"), strain_evidence_file=str(wr / "ev_species.tsv"))
    assert not os.path.exists(wr / "ev_species.tsv")
    _profile(eng, db, wr, gaf, species=False, strain=True, strain_evidence_file=str(wr / "ev.tsv"))
    assert open(wr / "ev.tsv", "rb").read() == open(wd / "ev.tsv", "rb").read()
    capfd.readouterr()
    _profile(eng, db, wr, gaf, species=True, strain=True, strain_evidence_file=str(wr / "ev_again.tsv"))
    assert not os.path.exists(wr / "ev_again.tsv") and "no strain step" in capfd.readouterr().err
    # several ranks
    for rank in range(2):
        wn = root / ("wd_ev_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, strain_evidence_file=str(wn / "ev.tsv"))
        assert e.value.code == E_INVALID
        assert not os.path.exists(wn / "ev.tsv") and not os.path.exists(wn / "species_abundance.txt")
