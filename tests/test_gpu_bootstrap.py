"""GPU tests of the bootstrap of the strain fit (pantax_hip_strain_bootstrap, --strain-bootstrap).  The rows and the weights of every replicate come from the
numpy restatement of the contract in tests/bootstrap_ref.py (pinned by tests/test_bootstrap_ref.py), applied to the bases_per_node that get_node_abundances
hands out; the reference of every LP is the oracle's own solver on the expanded rows (oracle.lad_solve / oracle.lad_objective).  Per (replicate, species):
rows_out and status exact, x >= 0, the objective of the device's x on the expanded rows equal to obj_out and both equal to the oracle's optimum to the
project's LP tolerance (rel 1e-9, abs 1e-12, tests/test_gpu_parity.py), x itself only where the two solutions agree to 1e-9 in L1 (the rule for non-unique
optima).  Everything that must not depend on the chunking, the route or the position of the species is compared bit for bit."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile, seam_world
from tests import bootstrap_ref as ref

pytestmark = pytest.mark.gpu

E_INVALID, E_LIMIT, E_SOLVER, E_STATE = -1, -4, -5, -7
SEED = 42


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _coverage(eng, sset):
    """the set resident with a coverage result of the stage kind -> bases_per_node; computed once per set"""
    if getattr(eng, "_boot_resident", None) is not sset:
        eng.upload_db(sset.species)
        eng.upload_packed(sset.reads)
        eng.rcls_profile(want_species=False)
        eng.trio_nodes_info()
        bases, _, _, _ = eng.get_node_abundances()
        sset._boot_bases = np.array(bases, copy=True)
        eng._boot_resident = sset
    return sset._boot_bases


def _visits(g):
    v = np.zeros((g.n_nodes, g.n_paths), dtype=bool)
    for h in range(g.n_paths):
        v[g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])], h] = True
    return v


def _selection(species, pick):
    """pick(s, H) -> the selected haplotypes of species s in column order -> (sel_off, sel_hap)"""
    off, hp = [0], []
    for s, g in enumerate(species):
        hp.extend(pick(s, g.n_paths))
        off.append(len(hp))
    return np.array(off, dtype=np.uint64), np.array(hp, dtype=np.uint32)


def _custom(name, node_len, paths, start, depth):
    """a species graph from explicit walks"""
    import synthdata as synth
    node_len = np.asarray(node_len, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.uint64)
    nodes = np.concatenate(paths).astype(np.uint32)
    glen = np.array([int(node_len[np.asarray(p)].sum()) for p in paths], dtype=np.int64)
    return synth.SpeciesGraph(name, node_len, off, nodes, ["GCF_%s_%03d" % (name, h) for h in range(len(paths))], start, start + len(node_len) - 1, glen,
                              np.asarray(depth, dtype=np.float64))


def _species_ref(g, bases, sel, key, b, seed=SEED):
    """the expanded rows of species g in replicate b over the selected haplotypes `sel` (column order): (mask, a) sorted"""
    member = _visits(g)[:, sel] if len(sel) else np.zeros((g.n_nodes, 0), dtype=bool)
    mask, a, v = ref.species_rows(g.node_len, bases, member)
    return ref.expand(mask, a, ref.weights(seed, key, b, v))


def _check_against_oracle(sset, bases, sel_off, sel_hap, keys, got, n_rep, seed=SEED):
    """every (replicate, species) of `got` against the reference rows and the oracle's solver; -> (LPs solved, LPs whose x was compared)"""
    from oracle import oracle as orc
    x, obj, rows, status = got
    S = len(sset.species)
    assert x.shape == (n_rep + 1, int(sel_off[-1])) and obj.shape == rows.shape == status.shape == (n_rep + 1, S)
    node_off = np.concatenate([[0], np.cumsum([g.n_nodes for g in sset.species])])
    n_solved = n_x = 0
    for s, g in enumerate(sset.species):
        c0, c1 = int(sel_off[s]), int(sel_off[s + 1])
        K = c1 - c0
        if K > 64:
            assert np.all(status[:, s] == E_LIMIT) and not rows[:, s].any() and not obj[:, s].any() and not x[:, c0:c1].any()
            continue
        sel = sel_hap[c0:c1].astype(np.int64)
        for b in range(n_rep + 1):
            m_exp, a_exp = _species_ref(g, bases[node_off[s]:node_off[s + 1]], sel, int(keys[s]), b, seed)
            n = len(a_exp)
            assert int(rows[b, s]) == n, (s, b)
            if K == 0 or n == 0:
                assert status[b, s] == 1 and obj[b, s] == 0.0 and not x[b, c0:c1].any(), (s, b)
                continue
            assert status[b, s] == 0, (s, b)
            xg = x[b, c0:c1]
            assert np.all(xg >= 0.0), (s, b)
            xo, objo, _, sto = orc.lad_solve(m_exp, a_exp, K, np.full(K, 1.05 * a_exp.max()))
            assert sto == 0
            assert orc.lad_objective(m_exp, a_exp, xg) * n == pytest.approx(obj[b, s], rel=1e-9, abs=1e-12), (s, b)
            assert obj[b, s] == pytest.approx(objo * n, rel=1e-9, abs=1e-12), (s, b, obj[b, s], objo * n)
            n_solved += 1
            if np.abs(xg - xo).sum() <= 1e-9:
                n_x += 1
    return n_solved, n_x


def _same(a, b):
    for p, q in zip(a, b):
        assert p.dtype == q.dtype and p.shape == q.shape and p.tobytes() == q.tobytes()


# ---- K_s in {1, 2, 3, 16, 17, 64, 65, 0}, a species without coverage; n_replicates 33, 1, 0; chunks of 1, 2 and all; both routes

@pytest.fixture(scope="module")
def mixed():
    import synthdata as synth
    rng = np.random.default_rng(931)
    haps = [1, 2, 3, 16, 17, 64, 65, 4, 5]
    species, start = [], 1
    for s, h in enumerate(haps):
        g = synth.make_species(rng, str(2000 + s), h, 8000 if h < 64 else 4000, start, "GCF_%06d" % (s + 1), present_frac=0.5)
        if s == 8:
            g.truth_depth[:] = 0.0                                           # no read of this species: no covered node
        species.append(g)
        start = g.range_end + 1
    sset = synth.SyntheticSet(species, synth.make_reads(rng, species, 6000))
    shuffle = np.random.default_rng(5)
    # every haplotype of the species in a shuffled order (column = position in the list, not haplotype index); none of species 7
    sset.sel = _selection(species, lambda s, H: [] if s == 7 else [int(h) for h in shuffle.permutation(H)])
    sset.keys = np.array([int(g.name) for g in species], dtype=np.uint64)
    return sset


N_REP = 33


@pytest.fixture(scope="module")
def mixed_run(eng, mixed):
    bases = _coverage(eng, mixed)
    return bases, eng.strain_bootstrap(*mixed.sel, mixed.keys, seed=SEED, n_replicates=N_REP)


def test_bootstrap_every_lp_against_the_oracle(eng, mixed, mixed_run):
    sset = mixed
    bases, got = mixed_run
    K = np.diff(sset.sel[0]).astype(int).tolist()
    assert K == [1, 2, 3, 16, 17, 64, 65, 0, 5]                                # both solver instances, their border, the limit, nothing selected
    assert all(200 <= g.n_nodes <= 2000 for g in sset.species[1:])
    x, obj, rows, status = got
    n_solved, n_x = _check_against_oracle(sset, bases, *sset.sel, sset.keys, got, N_REP)
    assert n_solved == 6 * (N_REP + 1) and n_x >= N_REP                        # the six covered species with 1 .. 64 columns in every replicate
    assert np.all(status[:, 6] == E_LIMIT) and np.all(status[:, 7] == 1) and np.all(status[:, 8] == 1) and not rows[:, 8].any()
    # replicate 0 has every row once: the nodes with coverage and a member, counted here from the graph
    node_off = np.concatenate([[0], np.cumsum([g.n_nodes for g in sset.species])])
    for s in range(6):
        g = sset.species[s]
        covered = bases[node_off[s]:node_off[s + 1]] > 0
        member = _visits(g)[:, sset.sel[1][int(sset.sel[0][s]):int(sset.sel[0][s + 1])].astype(int)].any(axis=1)
        assert int(rows[0, s]) == int((covered & member).sum()) > 0
    assert len({int(r) for r in rows[1:, 5]}) > 5                              # the replicates differ
    assert obj[1:, 5].std() > 0 and np.abs(x[1:] - x[0]).max() > 0


def test_bootstrap_chunks_routes_and_replicate_counts_same_bits(eng, mixed, mixed_run, set_opt):
    sset = mixed
    bases, got = mixed_run
    n_rows = int(got[2][0].sum())
    bound = n_rows + 8 * int(np.ceil(np.sqrt(n_rows))) + 64                    # bootstrap_rows_bound (tests/native/bootstrap_plan_check.cpp)
    for cap in (bound, 2 * bound, 3 * bound - 1):                              # one replicate a chunk; two; (all of them: the default above)
        set_opt(eng, "bootstrap_rows_max", cap)
        _same(eng.strain_bootstrap(*sset.sel, sset.keys, seed=SEED, n_replicates=N_REP), got)
    set_opt(eng, "bootstrap_rows_max", bound - 1)                              # not even one replicate: refused, and the reason says so
    from pantax_amd._ffi import PantaxHipError
    with pytest.raises(PantaxHipError) as e:
        eng.strain_bootstrap(*sset.sel, sset.keys, seed=SEED, n_replicates=N_REP)
    assert e.value.code == E_LIMIT and "bootstrap_rows_max" in str(e.value)
    set_opt(eng, "bootstrap_rows_max", None)
    set_opt(eng, "bootstrap_route", "walk")
    _same(eng.strain_bootstrap(*sset.sel, sset.keys, seed=SEED, n_replicates=N_REP), got)
    set_opt(eng, "bootstrap_route", None)
    for n in (0, 1):                                                           # a replicate does not depend on how many follow it
        _same(eng.strain_bootstrap(*sset.sel, sset.keys, seed=SEED, n_replicates=n), [a[:n + 1] for a in got])
    # two calls in a row, and a call behind the model fit on the same coverage result
    _same(eng.strain_bootstrap(*sset.sel, sset.keys, seed=SEED, n_replicates=3), [a[:4] for a in got])
    eng.strain_fit(sset.sel[0], sset.sel[1], np.ones(len(sset.sel[1])))
    _same(eng.strain_bootstrap(*sset.sel, sset.keys, seed=SEED, n_replicates=3), [a[:4] for a in got])
    # another seed draws other weights
    other = eng.strain_bootstrap(*sset.sel, sset.keys, seed=SEED + 1, n_replicates=1)
    assert np.array_equal(other[2][0], got[2][0]) and not np.array_equal(other[2][1], got[2][1])
    _same([a[:1] for a in other], [a[:1] for a in got])                        # the refit does not know the seed


# ---- membership edges: single-row patterns, a pattern of >= 3 000 equal abundances, a node walked twice by one haplotype

@pytest.fixture(scope="module")
def edges():
    import synthdata as synth
    rng = np.random.default_rng(932)
    species, start = [], 1
    # 0: 9 haplotypes, node v is walked by the haplotypes of the bits of v + 1: 500 nodes, 500 patterns of one row each
    V = 500
    paths = [[v for v in range(V) if (v + 1) >> k & 1] for k in range(9)]
    species.append(_custom("3000", np.full(V, 40), paths, start, [3.0] * 9))
    start = species[-1].range_end + 1
    # 1: one haplotype over 12 000 nodes of 2 bases: a = the number of reads over the node, thousands of rows with the same abundance in ONE pattern
    V = 12000
    species.append(_custom("3001", np.full(V, 2), [list(range(V))], start, [1.2]))
    start = species[-1].range_end + 1
    # 2: haplotype 0 comes back to node 7 and to node 150; haplotype 1 walks every third node
    V = 300
    walk0 = list(range(100)) + [7] + list(range(100, 200)) + [150] + list(range(200, V))
    species.append(_custom("3002", rng.integers(20, 60, V), [walk0, list(range(0, V, 3))], start, [4.0, 2.0]))
    sset = synth.SyntheticSet(species, synth.make_reads(rng, species, 3000, adversarial_frac=0.0))
    sset.sel = _selection(species, lambda s, H: list(range(H))[::-1] if s == 0 else list(range(H)))
    sset.keys = np.array([int(g.name) for g in species], dtype=np.uint64)
    return sset


def test_bootstrap_membership_edges(eng, edges, set_opt):
    sset = edges
    bases = _coverage(eng, sset)
    n_rep = 6
    got = eng.strain_bootstrap(*sset.sel, sset.keys, seed=7, n_replicates=n_rep)
    x, obj, rows, status = got
    # the borders, asserted from the set
    m0, a0 = _species_ref(sset.species[0], bases[:500], sset.sel[1][:9].astype(int), 3000, 0, 7)
    assert len(m0) > 300 and len(np.unique(m0)) == len(m0)                     # every pattern holds one row ...
    m1, _ = _species_ref(sset.species[0], bases[:500], sset.sel[1][:9].astype(int), 3000, 1, 7)
    assert len(np.unique(m1)) < 0.72 * len(m0)                                 # ... so about e^-1 of the patterns vanish in a replicate
    _, a_t = _species_ref(sset.species[1], bases[500:12500], np.array([0]), 3001, 0, 7)
    assert np.bincount(np.round(a_t * 2).astype(int)).max() >= 3000            # >= 3 000 rows of one abundance in the one pattern
    g2 = sset.species[2]
    w0 = g2.path_nodes[int(g2.path_off[0]):int(g2.path_off[1])]
    assert len(w0) == g2.n_nodes + 2 and bases[12500 + 7] > 0 and bases[12500 + 150] > 0
    n_solved, n_x = _check_against_oracle(sset, bases, *sset.sel, sset.keys, got, n_rep, seed=7)
    assert n_solved == 3 * (n_rep + 1) and n_x >= n_rep + 1                    # K = 1 is unique: x compared in every replicate of species 1
    set_opt(eng, "bootstrap_route", "walk")
    _same(eng.strain_bootstrap(*sset.sel, sset.keys, seed=7, n_replicates=n_rep), got)


# ---- the position of the species in the db

def test_bootstrap_species_position(eng):
    """the same species at index 0 of one db and at index 2 of another, under the same key: the same bits"""
    import synthdata as synth
    rng = np.random.default_rng(933)
    X = synth.make_species(rng, "4100", 5, 8000, 1, "GCF_X", present_frac=0.6)
    reads = synth.make_reads(rng, [X], 1500, adversarial_frac=0.0)
    A = synth.make_species(rng, "4101", 3, 6000, 1, "GCF_A", present_frac=0.5)
    B = synth.make_species(rng, "4102", 4, 6000, A.range_end + 1, "GCF_B", present_frac=0.5)
    shift = B.range_end
    X2 = dataclasses.replace(X, range_start=X.range_start + shift, range_end=X.range_end + shift)
    reads2 = dataclasses.replace(reads, node_id=(reads.node_id + np.uint32(shift)).astype(np.uint32))
    one, three = synth.SyntheticSet([X], reads), synth.SyntheticSet([A, B, X2], reads2)
    b1 = _coverage(eng, one)
    sel_x = [3, 0, 4, 1]
    r1 = eng.strain_bootstrap([0, 4], sel_x, [4100], seed=SEED, n_replicates=9)
    b3 = _coverage(eng, three)
    assert np.array_equal(b3[-X.n_nodes:], b1) and b1.any() and not b3[:-X.n_nodes].any()
    r3 = eng.strain_bootstrap([0, 2, 2, 6], [1, 0] + sel_x, [4101, 4102, 4100], seed=SEED, n_replicates=9)
    assert r3[0][:, 2:].tobytes() == r1[0].tobytes() and r3[1][:, 2].tobytes() == r1[1][:, 0].tobytes()
    assert np.array_equal(r3[2][:, 2], r1[2][:, 0]) and np.array_equal(r3[3][:, 2], r1[3][:, 0]) and np.all(r1[3] == 0)
    assert np.all(r3[3][:, :2] == 1) and r1[0].std(axis=0).max() > 0
    other = eng.strain_bootstrap([0, 2, 2, 6], [1, 0] + sel_x, [4101, 4102, 4103], seed=SEED, n_replicates=9)   # another key: other weights
    assert np.array_equal(other[2][0], r3[2][0]) and not np.array_equal(other[2][1:, 2], r3[2][1:, 2])


# ---- state and arguments

def _raw(eng, sel_off, sel_hap, keys, n_rep=2, n_species=None, null_key=False, fill=77):
    from pantax_amd import _ffi
    so, sh = np.ascontiguousarray(sel_off, dtype=np.uint64), np.ascontiguousarray(sel_hap, dtype=np.uint32)
    sk = np.ascontiguousarray(keys, dtype=np.uint64)
    cs = _ffi.BootstrapSet(eng.S if n_species is None else n_species, so.ctypes.data, sh.ctypes.data if len(sh) else None,
                           None if null_key else sk.ctypes.data, SEED, n_rep)
    R = n_rep + 1
    x = np.full((R, max(len(sh), 1)), float(fill))
    obj = np.full((R, eng.S), float(fill))
    rows = np.full((R, eng.S), fill, dtype=np.uint64)
    st = np.full((R, eng.S), fill, dtype=np.int32)
    rc = eng.lib.pantax_hip_strain_bootstrap(eng.ctx, eng.db, C.byref(cs), _ffi.p(x), _ffi.p(obj), _ffi.p(rows), _ffi.p(st))
    return rc, (x, obj, rows, st)


def _untouched(out, fill=77):
    return all(np.all(a == fill) for a in out)


def test_bootstrap_state_and_arguments(eng, mixed):
    from pantax_amd._ffi import PantaxHipError
    sset = mixed
    eng._boot_resident = None
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    sel_off, sel_hap = sset.sel
    rc, out = _raw(eng, sel_off, sel_hap, sset.keys)
    assert rc == E_STATE and _untouched(out)                                   # no coverage pass yet
    eng.get_node_abundances(fetch=False)
    rc, out = _raw(eng, sel_off, sel_hap, sset.keys)
    assert rc == 0 and not _untouched(out)
    good = out
    twice = sel_hap.copy()
    twice[2] = twice[1]                                                        # species 1: a haplotype twice
    beyond = sel_hap.copy()
    beyond[0] = 1                                                              # species 0 has one haplotype
    for args, kw in (((sel_off, twice, sset.keys), {}), ((sel_off, beyond, sset.keys), {}),
                     ((sel_off[:-1], sel_hap[:int(sel_off[-2])], sset.keys[:-1]), {"n_species": eng.S - 1}),
                     ((sel_off, sel_hap, sset.keys), {"null_key": True})):
        rc, out = _raw(eng, *args, **kw)
        assert rc == E_INVALID and _untouched(out)
    eng.profile_step(sset.avg_len())                                           # a resident step may zero the arena
    with pytest.raises(PantaxHipError) as e:
        eng.strain_bootstrap(sel_off, sel_hap, sset.keys, n_replicates=2)
    assert e.value.code == E_STATE and "resident step" in str(e.value)
    rc, out = _raw(eng, sel_off, sel_hap, sset.keys)
    assert rc == E_STATE and _untouched(out)
    eng.get_node_abundances(fetch=False)
    _same(eng.strain_bootstrap(sel_off, sel_hap, sset.keys, seed=SEED, n_replicates=2), good)


# ---- the file seam -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world(tmp_path_factory):
    yield from seam_world(tmp_path_factory, "pantax_boot", 32, 4, 5, 30000, 30000, present_frac=0.4, single_strain_every=4, with_ids=True)


HEADER = ["species_taxid", "strain_taxid", "genome_ID", "class", "predicted_coverage", "refit", "n_solved", "mean", "sd", "q025", "q25", "q50", "q75", "q975", "min",
          "zero_fraction", "share", "share_q025", "share_q975", "n_rows", "objective"]
N_SEAM = 8


def _stats_cells(x, status):
    """the cells n_solved .. zero_fraction of one summary, as parsed values ("-" where nothing was solved)"""
    from pantax_amd.engine import bootstrap_summary
    o = bootstrap_summary(x, status)
    return o, [int(o[0])] + [np.float64(o[i]) if o[0] > 0 else "-" for i in (1, 2, 3, 4, 5, 6, 7, 9, 8)]


def _parsed(cells):
    return [c if c == "-" else np.float64(c) for c in cells]


def test_profile_seam_strain_bootstrap(world, set_opt, monkeypatch):
    from pantax_amd import _ffi
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng = world
    _profile(eng, db, root / "wd_plain", gaf)
    wd = root / "wd_boot"
    set_opt(eng, "db_groups", 1)
    _profile(eng, db, wd, gaf, strain_bootstrap_file=str(wd / "boot.tsv"), strain_bootstrap_replicates=N_SEAM)
    for f in ("species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt"):   # the option changes none of the tables
        assert open(wd / f, "rb").read() == open(root / "wd_plain" / f, "rb").read()
    assert not os.path.exists(root / "wd_plain" / "boot.tsv")
    rows = _lines(wd / "boot.tsv")
    assert rows[0] == HEADER and all(len(r) == len(HEADER) for r in rows)
    rows = rows[1:]
    table = _lines(wd / "strain_abundance.txt")[1:]
    n_str = len(table)
    assert n_str >= 2 and [tuple(r[:4]) for r in rows[:n_str]] == [tuple(t[:3]) + ("strain",) for t in table]
    assert all(np.float64(rows[i][4]) == np.float64(table[i][3]) for i in range(n_str))
    sp_rows = rows[n_str:]
    assert all(r[1] == "-" and r[2] == "-" and r[3] == "species" for r in sp_rows)
    # the stage call of the same sample for the table's rows, the species taxids as keys, the sampler's seed
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    eng.get_node_abundances(fetch=False)
    names = [g.name for g in sset.species]
    genome_hap = {r[0]: r[0].split("_ASM")[0] for r in _lines(db / "genomes_info.txt")[1:]}
    picked = [[] for _ in names]                                             # per species: (haplotype, row of the table), ascending haplotype = column order
    for i, t in enumerate(table):
        s = names.index(t[0])
        picked[s].append((sset.species[s].hap_names.index(genome_hap[t[2]]), i))
    for p in picked:
        p.sort()
    sel_off = np.concatenate([[0], np.cumsum([len(p) for p in picked])]).astype(np.uint64)
    sel_hap = np.array([h for p in picked for h, _ in p], dtype=np.uint32)
    x, obj, nrows, status = eng.strain_bootstrap(sel_off, sel_hap, [int(n) for n in names], seed=42, n_replicates=N_SEAM)
    entry_of_row = {i: (s, int(sel_off[s]) + k) for s, p in enumerate(picked) for k, (_, i) in enumerate(p)}
    n_moved = 0
    for i in range(n_str):
        s, e = entry_of_row[i]
        c0, c1 = int(sel_off[s]), int(sel_off[s + 1])
        assert status[0, s] == 0
        r = rows[i]
        assert np.float64(r[5]) == x[0, e]
        o, cells = _stats_cells(x[1:, e], status[1:, s])
        assert [int(r[6])] + _parsed(r[7:16]) == cells
        seq_tot = np.zeros(N_SEAM + 1)
        for c in range(c0, c1):                                              # the species' columns added in order
            seq_tot = seq_tot + x[:, c]
        share = np.where(seq_tot == 0, 0.0, x[:, e] / np.where(seq_tot == 0, 1.0, seq_tot))
        assert np.float64(r[16]) == share[0]
        os_, _ = _stats_cells(share[1:], status[1:, s])
        assert np.float64(r[17]) == os_[3] and np.float64(r[18]) == os_[7] and r[19] == "-" and r[20] == "-"
        n_moved += int(o[2] > 0)
    assert n_moved >= 1                                                      # some strain's coverage moves between the replicates
    seq = [r[0] for r in sp_rows]
    sp_table = [r[0] for r in _lines(wd / "species_abundance.txt")[1:]]      # the run takes the selected species in the order of the species table
    assert len(set(seq)) == len(seq) >= 2 and seq == [t for t in sp_table if t in set(seq)] and {t[0] for t in table} <= set(seq)
    for r in sp_rows:
        s = names.index(r[0])
        assert int(r[19]) == int(nrows[0, s]) and np.float64(r[20]) == obj[0, s] and r[4] == "-" and r[5] == "-" and r[15:19] == ["-"] * 4
        _, cells = _stats_cells(obj[1:, s], status[1:, s])
        assert [int(r[6])] + _parsed(r[7:15]) == cells[:9]
    # the same file from a run cut into three groups of species
    wg = root / "wd_boot_groups"
    set_opt(eng, "db_groups", 3)
    _profile(eng, db, wg, gaf, strain_bootstrap_file=str(wg / "boot.tsv"), strain_bootstrap_replicates=N_SEAM)
    set_opt(eng, "db_groups", None)
    assert open(wg / "boot.tsv", "rb").read() == open(wd / "boot.tsv", "rb").read()
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_boot_cli"
    wc.mkdir()
    run = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0",
                          "--strain-bootstrap", str(wc / "boot.tsv"), "--strain-bootstrap-replicates", str(N_SEAM)], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert open(wc / "boot.tsv", "rb").read() == open(wd / "boot.tsv", "rb").read()
    # another seed: other replicates, the same refit
    ws = root / "wd_boot_seed"
    _profile(eng, db, ws, gaf, strain_bootstrap_file=str(ws / "boot.tsv"), strain_bootstrap_replicates=N_SEAM, strain_bootstrap_seed=43)
    other = _lines(ws / "boot.tsv")[1:]
    assert [r[:6] for r in other] == [r[:6] for r in rows] and other != rows
    # several ranks: refused with the plan's wording
    for rank in range(2):
        wn = root / ("wd_boot_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, strain_bootstrap_file=str(wn / "boot.tsv"))
        assert e.value.code == E_INVALID and "the bootstrap report (strain_bootstrap_file) needs one rank and an unsharded ingest (world_size 2)" in str(e.value)
        assert not os.path.exists(wn / "boot.tsv") and not os.path.exists(wn / "species_abundance.txt")
    # a caller compiled against the header before the bootstrap fields: its struct ends behind strain_fit_file, the report reads as off
    real = _ffi.ProfileExt

    class OldExt(real):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.struct_size = 16

    monkeypatch.setattr(_ffi, "ProfileExt", OldExt)
    wo = root / "wd_boot_old"
    _profile(eng, db, wo, gaf, strain_fit_file=str(wo / "fit.tsv"), strain_bootstrap_file=str(wo / "boot.tsv"), strain_bootstrap_replicates=N_SEAM)
    monkeypatch.setattr(_ffi, "ProfileExt", real)
    assert os.path.exists(wo / "fit.tsv") and not os.path.exists(wo / "boot.tsv")
    assert open(wo / "strain_abundance.txt", "rb").read() == open(wd / "strain_abundance.txt", "rb").read()
