"""GPU tests of the per-strain read support (pantax_hip_strain_read_support, --strain-read-support).  The expected integers come from the row-by-row
reading of the contract in tests/read_support_ref.py (pinned by hand in tests/test_read_support_ref.py); everything compares element for element."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile, seam_world
from tests.read_support_ref import check_identities, read_support

pytestmark = pytest.mark.gpu

WALK_STEPS = (1, 2, 63, 64, 65, 130)   # in-group decide, a walk that ends on lane 63, the long kernel with two and three partials


def _build():
    """Ten species: four tiny ones (their reads share one 64-step group with their neighbours'), K_s = 1, K_s = 2 with equal weights, a 64-haplotype
    species with all 64 as candidates (bit 63), a 70-haplotype species with 66 candidates (two mask words, no pair block), a species without
    candidates, and one that is left out of the db (its reads are "U").  Short reads of the generator plus hand-placed walks."""
    import synthdata as synth
    rng = np.random.default_rng(5)
    shapes = [(2, 250), (3, 250), (2, 250), (3, 250), (1, 8000), (4, 8000), (64, 8000), (70, 8000), (3, 6000), (3, 6000)]
    species, start = [], 1
    for i, (H, glen) in enumerate(shapes):
        g = synth.make_species(rng, str(1000 + i), H, glen, start, "GCF_%06d" % (i + 1), present_frac=0.6)
        species.append(g)
        start = g.range_end + 1
    rd = synth.make_reads(rng, species[4:], 2500, adversarial_frac=0.0)
    walks, ps, pe = [], [], []

    def add(g, local_nodes, pstart=3, pend=40):
        walks.append(np.asarray(local_nodes, dtype=np.uint32) + np.uint32(g.range_start))
        ps.append(pstart)
        pe.append(pend)

    def stretch(g, h, k, at=0):
        b = int(g.path_off[h])
        assert int(g.path_off[h + 1]) - b >= at + k
        return g.path_nodes[b + at:b + at + k]

    for g in species[:4]:                                # three or more species inside the first 64-step group
        add(g, stretch(g, 0, 1), 0, 11)
        add(g, stretch(g, g.n_paths - 1, 2, at=3), 5, 9)
    for g in (species[5], species[6], species[7]):
        for k in WALK_STEPS:
            for h in (0, g.n_paths - 1):
                add(g, stretch(g, h, k, at=7), 2, 2 + 31 * k)
    two = species[5]
    a, b = stretch(two, 1, 2, at=20)
    add(two, [a, b, a, b, a])                            # a walk that visits a node twice (and more)
    add(two, stretch(two, 0, 3), 90, 10)                 # pend < pstart: span 0
    add(two, [0, two.n_nodes - 1, two.n_nodes // 2])     # unlikely to fit any candidate
    add(species[4], stretch(species[4], 0, 4))
    k = np.array([len(w) for w in walks], dtype=np.uint64)
    n = len(walks)
    one = lambda v: np.full(n, v, dtype=np.int64)
    reads = synth.PackedReads(np.concatenate([rd.step_off, rd.step_off[-1] + np.cumsum(k)]), np.concatenate([rd.node_id] + walks), None,
                              np.concatenate([rd.pstart, np.array(ps, dtype=np.int64)]), np.concatenate([rd.pend, np.array(pe, dtype=np.int64)]),
                              np.concatenate([rd.qlen, one(30000)]), np.concatenate([rd.mapq, one(60)]), np.concatenate([rd.plen, one(30000)]))
    R = reads.n_reads
    flags = np.zeros(R, dtype=np.uint8)
    flags[rng.choice(R, size=60, replace=False)] = rng.choice([1, 2], size=60).astype(np.uint8)
    flags[R - 3] = 1                                      # a dropped hand-placed read
    db = species[:9]                                      # the last species is not in the db
    picks = [[0, 1], [1], [], [2, 0, 1], [0], [2, 0], list(range(63, -1, -1)), sorted(rng.choice(70, size=66, replace=False).tolist()), []]
    weights = [[1.0, 2.0], [4.0], [], [3.0, 3.0, 3.0], [1.5], [2.5, 2.5], rng.choice([1.0, 2.5, 7.25], size=64).tolist(),
               (rng.random(66) * 10 + 0.1).tolist(), []]
    off = np.cumsum([0] + [len(x) for x in picks]).astype(np.uint64)
    cands = (off, np.array(sum(picks, []), dtype=np.uint32), np.array(sum(weights, []), dtype=np.float64))
    return db, reads, flags, cands


def _reference(db, reads, flags, cands):
    from oracle import oracle as orc
    sp = orc.bin_reads(reads.step_off, reads.node_id, [g.range_start for g in db], [g.range_end for g in db])
    hap_nodes = [[set(g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])].tolist()) for h in range(g.n_paths)] for g in db]
    so = reads.step_off.astype(np.int64)
    rows = []
    for r in range(reads.n_reads):
        s = int(sp[r])
        nodes = (reads.node_id[so[r]:so[r + 1]].astype(np.int64) - db[s].range_start).tolist() if s >= 0 else []
        rows.append((s, flags[r] == 0, nodes, int(reads.pstart[r]), int(reads.pend[r])))
    return sp, read_support(hap_nodes, rows, *cands)


@pytest.fixture(scope="module")
def stage():
    from pantax_amd.engine import Engine
    db, reads, flags, cands = _build()
    sp, exp = _reference(db, reads, flags, cands)
    eng = Engine(0)
    eng.upload_db(db)
    eng.upload_reads(reads.step_off, reads.node_id, reads.pstart, reads.pend, reads.qlen, reads.mapq, flags)
    eng.rcls_profile(want_species=False)
    yield eng, db, reads, flags, cands, sp, exp
    eng.close()


def _same(got, exp):
    for g, e in zip(got, exp):
        assert g.dtype == np.uint64 and g.shape == e.shape
        assert np.array_equal(g, e)


def test_stage_call_equals_reference(stage, set_opt):
    eng, db, reads, flags, cands, sp, exp = stage
    k = np.diff(reads.step_off.astype(np.int64))
    for steps in WALK_STEPS:
        assert (k == steps).sum() >= 6
    assert (sp < 0).sum() > 5 and ((sp >= 0) & (flags != 0)).sum() > 10             # "U" reads, dropped reads
    hap, species, pair_off, pair = exp
    assert species[2, 0, 0] == 2 and not species[2, 1:].any() and species[8, 0, 0] > 10 and not species[8, 1:].any()   # K_s = 0: counted only
    assert species[:, 1, 0].sum() > 0 and species[:, 2, 0].sum() > 100 and species[:, 3, 0].sum() > 0
    assert hap[int(cands[0][6]), 0, 0] > 0                                           # haplotype 63 of the 64-haplotype species: bit 63
    assert pair_off[8] == pair_off[7] and pair_off[7] - pair_off[6] == 64 * 64        # 66 candidates: no block
    check_identities(*exp, cands[0])
    got = eng.strain_read_support(*cands)
    _same(got, exp)
    set_opt(eng, "read_strain_route", "walk")                                        # every species through the compact walk masks
    _same(eng.strain_read_support(*cands), exp)


def test_pair_matrix_and_identities(stage):
    eng, db, reads, flags, cands, sp, exp = stage
    hap, species, pair_off, pair = eng.strain_read_support(*cands)
    check_identities(hap, species, pair_off, pair, cands[0])
    shared = 0
    for s in range(len(db)):
        K = int(cands[0][s + 1] - cands[0][s])
        if K == 0 or K > 64:
            assert pair_off[s + 1] == pair_off[s]
            continue
        m = pair[int(pair_off[s]):int(pair_off[s + 1])].reshape(K, K)
        assert np.array_equal(m, m.T)
        assert np.array_equal(np.diag(m), hap[int(cands[0][s]):int(cands[0][s + 1]), 0, 0])
        shared += int(np.triu(m, 1).sum())
    assert shared > 100


def test_cross_check_with_read_strains(stage):
    """assigned, unique, unexplained and counted against the per-read arrays of the merged per-read assignment on the same inputs"""
    eng, db, reads, flags, cands, sp, exp = stage
    hap, species, _, _ = eng.strain_read_support(*cands)
    rh, rn, _ = eng.read_strains(*cands)
    off, ch, _ = cands
    for s in range(len(db)):
        mine = sp == s
        K = int(off[s + 1] - off[s])
        if K == 0:
            assert species[s, 0, 0] == (mine & (flags == 0)).sum()
            continue
        assert species[s, 0, 0] == (mine & (rn >= 0)).sum()
        assert species[s, 1, 0] == (mine & (rn == 0)).sum()
        for c in range(int(off[s]), int(off[s + 1])):
            assert hap[c, 2, 0] == (mine & (rn > 0) & (rh == ch[c])).sum()
            assert hap[c, 1, 0] == (mine & (rn == 1) & (rh == ch[c])).sum()


def test_empty_candidate_set(stage):
    eng, db, reads, flags, cands, sp, exp = stage
    S = len(db)
    hap, species, pair_off, pair = eng.strain_read_support(np.zeros(S + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0))
    assert hap.shape == (0, 3, 3) and pair.shape == (0,) and not pair_off.any()
    assert np.array_equal(species[:, 0], exp[1][:, 0]) and not species[:, 1:].any()


def _raw(eng, cands, n_species=None, pair_cap=None):
    from pantax_amd import _ffi
    from pantax_amd.engine import p
    off, ch, cw = cands
    S = eng.S
    cs = _ffi.ReadStrainSet(S if n_species is None else n_species, off.ctypes.data, ch.ctypes.data, cw.ctypes.data)
    k = np.diff(off.astype(np.int64))
    n_pair = int((k[k <= 64] ** 2).sum())
    hap = np.full((len(ch), 3, 3), 77, dtype=np.uint64)
    species = np.full((S, 4, 3), 77, dtype=np.uint64)
    pair_off = np.full(S + 1, 77, dtype=np.uint64)
    pair = np.full(max(n_pair, 1), 77, dtype=np.uint64)
    rc = eng.lib.pantax_hip_strain_read_support(eng.ctx, eng.db, eng.reads, C.byref(cs), p(hap), p(species), p(pair_off), n_pair if pair_cap is None else pair_cap, p(pair))
    return rc, hap, species, pair_off, pair


def test_sizing_and_arguments(stage):
    from pantax_amd import _ffi
    from pantax_amd._ffi import PantaxHipError
    eng, db, reads, flags, cands, sp, exp = stage
    rc, hap, species, pair_off, pair = _raw(eng, cands, pair_cap=0)
    assert rc == _ffi.E_LIMIT
    assert np.array_equal(pair_off, exp[2])                                           # the sizes are out ...
    assert np.all(hap == 77) and np.all(species == 77) and np.all(pair == 77)         # ... and nothing else is touched
    rc, hap, species, pair_off, pair = _raw(eng, cands)
    assert rc == 0
    _same((hap, species, pair_off, pair), exp)
    off, ch, cw = cands
    twice = ch.copy()
    twice[int(off[3]) + 1] = twice[int(off[3])]                                       # a haplotype twice within a species
    far = ch.copy()
    far[int(off[0])] = 2                                                              # species 0 has two haplotypes
    for bad in ((off, twice, cw), (off, far, cw)):
        with pytest.raises(PantaxHipError) as e:
            eng.strain_read_support(*bad)
        assert e.value.code == -1
    assert _raw(eng, cands, n_species=eng.S + 1)[0] == -1


def test_state(stage):
    """reads binned against another db are refused, as by pantax_hip_read_strains"""
    from pantax_amd._ffi import PantaxHipError
    from pantax_amd.engine import Engine
    eng, db, reads, flags, cands, sp, exp = stage
    with Engine(0) as e2:
        e2.upload_db(db)
        e2.upload_reads(reads.step_off, reads.node_id, reads.pstart, reads.pend, reads.qlen, reads.mapq, flags)
        with pytest.raises(PantaxHipError) as e:
            e2.strain_read_support(*cands)                 # not binned yet
        assert e.value.code == -7
        e2.rcls_profile(want_species=False)
        e2.upload_db(db)                                   # a new db: the reads were binned against the previous one
        with pytest.raises(PantaxHipError) as e:
            e2.strain_read_support(*cands)
        assert e.value.code == -7
        with pytest.raises(PantaxHipError) as e:
            e2.read_strains(*cands)
        assert e.value.code == -7


# ---- the file seam -----------------------------------------------------------------------------------------------------------

HEADER = ["species_taxid", "strain_taxid", "genome_ID", "class", "n_reads", "n_steps", "span", "fraction", "other_strain_taxid"]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    yield from seam_world(tmp_path_factory, "pantax_sup", 37, 2, 5, 12000, 30000, present_frac=0.6, with_ids=True)


def test_profile_seam_read_support(world, capfd):
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng = world
    plain = root / "wd_plain"
    _profile(eng, db, plain, gaf)
    wd = root / "wd_sup"
    _profile(eng, db, wd, gaf, strain_read_support_file=str(wd / "sup.tsv"))
    for f in ("species_abundance.txt", "strain_abundance.txt"):       # the option changes none of the tables
        assert open(wd / f, "rb").read() == open(plain / f, "rb").read()
    assert not os.path.exists(plain / "sup.tsv")
    rows = _lines(wd / "sup.tsv")
    assert rows[0] == HEADER
    body = rows[1:]
    # the candidates from the tables, as the per-read report's test takes them: the rows of strain_abundance.txt, weight = predicted_coverage
    gi = _lines(db / "genomes_info.txt")[1:]
    genome_hap = {r[0]: r[0].split("_ASM")[0] for r in gi}
    names = [g.name for g in sset.species]
    table = _lines(wd / "strain_abundance.txt")[1:]
    cand = {s: [] for s in range(len(names))}
    for r in table:
        s = names.index(r[0])
        h = sset.species[s].hap_names.index(genome_hap[r[2]])
        if h not in [x[0] for x in cand[s]]:                          # (a haplotype's first row stands for it)
            cand[s].append((h, float(r[3]), r[1]))
    assert all(len(cand[s]) >= 2 for s in cand)
    for s in cand:
        cand[s].sort()                                                # ascending haplotype index: the seam's candidate lists
    off = np.cumsum([0] + [len(cand[s]) for s in range(len(names))]).astype(np.uint64)
    ch = np.array([h for s in range(len(names)) for h, _, _ in cand[s]], dtype=np.uint32)
    cw = np.array([w for s in range(len(names)) for _, w, _ in cand[s]], dtype=np.float64)
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    hap, species, pair_off, pair = eng.strain_read_support(off, ch, cw)
    assert hap[:, 1, 0].sum() > 0 and species[:, 2, 0].sum() > 0
    # 1. the strain rows in the order of strain_abundance.txt, three classes each
    n_strain = 3 * len(table)
    entry = {(s, h): int(off[s]) + i for s in cand for i, (h, _, _) in enumerate(cand[s])}
    for i, r in enumerate(table):
        s = names.index(r[0])
        e = entry[(s, sset.species[s].hap_names.index(genome_hap[r[2]]))]
        for j, cls in enumerate(("compatible", "unique", "assigned")):
            row = body[3 * i + j]
            assert row[:4] == [r[0], r[1], r[2], cls] and row[8] == "-"
            assert [int(x) for x in row[4:7]] == hap[e, j].tolist()
            assert float(row[7]) == float(hap[e, j, 0]) / float(species[s, 0, 0])
    # 2. the species rows in shard order, four classes each
    at = n_strain
    for s in range(len(names)):
        for j, cls in enumerate(("counted", "unexplained", "ambiguous", "uninformative")):
            row = body[at]
            at += 1
            assert row[:4] == [names[s], "-", "-", cls] and row[8] == "-"
            assert [int(x) for x in row[4:7]] == species[s, j].tolist()
    # 3. the shared rows: every pair a < b with a non-zero count
    exp_shared = []
    for s in range(len(names)):
        K = len(cand[s])
        m = pair[int(pair_off[s]):int(pair_off[s + 1])].reshape(K, K)
        for a in range(K):
            for b in range(a + 1, K):
                if m[a, b]:
                    exp_shared.append((names[s], cand[s][a][2], "shared", int(m[a, b]), float(m[a, b]) / float(min(m[a, a], m[b, b])), cand[s][b][2]))
    assert len(exp_shared) > 0 and len(body) == at + len(exp_shared)
    for row, e in zip(body[at:], exp_shared):
        assert (row[0], row[1], row[3], int(row[4]), float(row[7]), row[8]) == e and row[5] == row[6] == "-"
    full = open(wd / "sup.tsv", "rb").read()
    # a species-only run writes nothing; the strain-only resume behind it writes the same file
    wr = root / "wd_sup_resume"
    capfd.readouterr()
    _profile(eng, db, wr, gaf, species=True, strain=False, out_binning_file=str(wr / "reads_classification.tsv"),
             strain_read_support_file=str(wr / "sup_species_only.tsv"))
    assert not os.path.exists(wr / "sup_species_only.tsv") and "no strain step" in capfd.readouterr().err
    _profile(eng, db, wr, gaf, species=False, strain=True, strain_read_support_file=str(wr / "sup.tsv"))
    assert open(wr / "sup.tsv", "rb").read() == full
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_sup_cli"
    wc.mkdir()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0",
                        "--strain-read-support", str(wc / "sup.tsv")], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc / "sup.tsv", "rb").read() == full
    # several ranks: refused on every rank, before any collective
    for rank in range(2):
        wn = root / ("wd_sup_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, strain_read_support_file=str(wn / "sup.tsv"))
        assert e.value.code == -1
        assert not os.path.exists(wn / "sup.tsv")
