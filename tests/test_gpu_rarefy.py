"""GPU tests of the rarefaction of the strain fit (pantax_hip_strain_rarefy, pantax_hip_rarefy_node_bases, --strain-rarefy).  The pass over the reads is
pinned against the existing coverage pass on the crafted walks of tests/cov_walk_cases.py (thinned-out reads as drop flags) and against the C oracle; the
stage call against the plain-Python reference of tests/rarefy_ref.py (pinned by tests/test_rarefy_ref.py): rows, status, reads and member counts exact, every
LP against the oracle's solver to the project's LP tolerance (rel 1e-9, abs 1e-12, tests/test_gpu_parity.py), x itself only where the two solutions agree to
1e-9 in L1.  Everything that must not depend on the levels a pass serves, the route or the position of the species is compared bit for bit."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import oracle_coverage, seam_lines as _lines, seam_profile as _profile, seam_world
from tests import cov_walk_cases as cw
from tests import rarefy_ref as ref

pytestmark = pytest.mark.gpu

E_INVALID, E_LIMIT, E_SOLVER, E_STATE = -1, -4, -5, -7
NULLFIELD, DUPDROP = 1, 2
SEED = 42


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _same(a, b):
    for p, q in zip(a, b):
        assert p.dtype == q.dtype and p.shape == q.shape and p.tobytes() == q.tobytes()


# ---- 1. the pass over the reads against the existing coverage pass, exact

def _crafted():
    """the corpus of cov_walk_cases with walks of 65 and 130 steps, reads of no species and pre-flagged reads on top -> (species, reads, flags)"""
    import synthdata as synth
    species, rd, _ = cw.build()
    A, B, Cs = species
    lens = np.zeros(Cs.range_end + 2, dtype=np.int64)
    for g in species:
        lens[g.range_start:g.range_end + 1] = g.node_len
    extra = []

    def add(walk, ps, pe=None):
        walk = np.asarray(walk, dtype=np.int64)
        extra.append((walk, ps, int(lens[walk].sum()) if pe is None else pe))
    for ps in (0, 1):
        add(3300 + np.arange(65), ps)
        add(3400 + np.arange(130), ps)
        add(9700 - np.arange(130), ps)
        add(np.concatenate([11300 + np.arange(100), 11300 + np.arange(30)]), ps)      # 130 steps, the last 30 walked before
        add(np.concatenate([5000 + np.arange(64), [5000]]), ps)                        # 65 steps, the last is step 0 again
    w = 6200 + np.arange(130)
    add(w, 0, int(lens[w[:100]].sum()))                                                # the target ends long before the last step
    add(w, 3, 1)                                                                       # pend < pstart
    add(w, int(lens[w[0]]) + 1)                                                        # pstart beyond the first node: an abort
    add(6500 + np.arange(66), int(lens[6500]))                                         # nothing of the first node
    add([A.range_end, B.range_start], 0)                                               # of no species
    add([B.range_end - 1, B.range_end, Cs.range_start, Cs.range_start + 1], 0)
    add(np.concatenate([B.range_end - np.arange(70), [Cs.range_start]]), 0)            # ... and a long one
    n0, n = rd.n_reads, rd.n_reads + len(extra)
    so = np.concatenate([rd.step_off.astype(np.int64), int(rd.step_off[-1]) + np.cumsum([len(e[0]) for e in extra])]).astype(np.uint64)
    reads = synth.PackedReads(so, np.concatenate([rd.node_id] + [e[0].astype(np.uint32) for e in extra]), np.zeros(int(so[-1]), np.uint8),
                              np.concatenate([rd.pstart, [e[1] for e in extra]]).astype(np.int64), np.concatenate([rd.pend, [e[2] for e in extra]]).astype(np.int64),
                              np.full(n, 150, np.int64), np.full(n, 60, np.int64), np.zeros(n, np.int64))
    flags = np.zeros(n, dtype=np.uint8)
    flags[5::97] = NULLFIELD
    flags[11::89] |= DUPDROP
    flags[n0 + 1] = DUPDROP                                                            # a walk of 130 steps among the pre-flagged
    return species, reads, flags


def test_node_bases_equal_the_coverage_pass_on_thinned_reads(eng):
    from oracle import oracle as orc
    species, rd, flags0 = _crafted()
    k = np.diff(rd.step_off.astype(np.int64))
    assert (k == 65).sum() >= 5 and (k == 130).sum() >= 8 and (flags0 == NULLFIELD).sum() > 5 and (flags0 & DUPDROP).astype(bool).sum() > 5
    eng.upload_db(species)
    eng.upload_packed(rd, flags=flags0)

    def coverage():
        sp, *_ = eng.rcls_profile()
        eng.trio_nodes_info(fetch=False)
        return sp, np.asarray(eng.get_node_abundances(with_trio=False)[0]).astype(np.uint64)
    sp, bases0 = coverage()
    assert (sp < 0).sum() >= 5 and len(np.unique(sp[sp >= 0])) == 3
    # level 0 is every counted read: the coverage pass itself, and the oracle's result
    exp = oracle_coverage(species, rd, orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in species], [g.range_end for g in species]), keep=flags0 == 0)
    oracle_bases = np.concatenate([r[1] for r in exp]).astype(np.uint64)
    assert np.array_equal(bases0, oracle_bases) and sum(r[4] for r in exp) > 0
    got = {(b, l): eng.rarefy_node_bases(SEED, b, l) for b in (1, 2) for l in (0, 1, 3)}   # all of them before any flag changes
    for b in (1, 2):
        bad = np.nonzero(got[b, 0] != bases0)[0]
        assert len(bad) == 0, "level 0 of replicate %d differs at %d nodes, first %s: got %s, coverage pass %s" % (
            b, len(bad), bad[:8].tolist(), got[b, 0][bad[:8]].tolist(), bases0[bad[:8]].tolist())
    assert np.array_equal(eng.rarefy_node_bases(SEED, 0, 0), bases0)                       # replicate 0 is allowed in the seam
    try:
        for b in (1, 2):
            d = ref.depths(SEED, b, rd.n_reads)
            for l in (1, 3):
                flags = flags0.copy()
                flags[d < l] |= DUPDROP
                assert 0 < (flags == 0).sum() < (flags0 == 0).sum()
                eng.set_read_flags(flags)
                _, thin = coverage()
                bad = np.nonzero(got[b, l] != thin)[0]
                assert len(bad) == 0, "level %d of replicate %d differs at %d nodes, first %s: got %s, coverage pass %s" % (
                    l, b, len(bad), bad[:8].tolist(), got[b, l][bad[:8]].tolist(), thin[bad[:8]].tolist())
                assert thin.sum() < bases0.sum()
        assert not np.array_equal(got[1, 1], got[2, 1]) and got[1, 3].sum() < got[1, 1].sum()
    finally:
        eng.set_read_flags(flags0)
    _, again = coverage()
    assert np.array_equal(again, bases0)
    assert np.array_equal(eng.rarefy_node_bases(SEED, 1, 1), got[1, 1])                    # the same bits on every run


# ---- 2. the stage call on a small mixed set: K_s in {1, 2, 3, 64, 65, 0} and a species without reads

N_LEVELS, N_REP = 12, 3


def _selection(species, pick):
    off, hp = [0], []
    for s, g in enumerate(species):
        hp.extend(pick(s, g.n_paths))
        off.append(len(hp))
    return np.array(off, dtype=np.uint64), np.array(hp, dtype=np.uint32)


@pytest.fixture(scope="module")
def mixed():
    import synthdata as synth
    from oracle import oracle as orc
    rng = np.random.default_rng(941)
    haps = [1, 2, 3, 64, 65, 4, 5]
    species, start = [], 1
    for s, h in enumerate(haps):
        g = synth.make_species(rng, str(5000 + s), h, 8000 if h < 64 else 4000, start, "GCF_%06d" % (s + 1), present_frac=0.5)
        g.truth_depth[:] = 0.0 if s == 6 else 1.0 / float(g.genome_len.sum())   # the same share of the reads for every species but the last: none of it
        species.append(g)
        start = g.range_end + 1
    sset = synth.SyntheticSet(species, synth.make_reads(rng, species, 2400, adversarial_frac=0.0))
    shuffle = np.random.default_rng(6)
    sset.sel = _selection(species, lambda s, H: [] if s == 5 else [int(h) for h in shuffle.permutation(H)])   # shuffled columns; none of species 5
    rd = sset.reads
    sset.sp = orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in species], [g.range_end for g in species])
    sset.ref = ref.stage_reference(species, rd, sset.sp, np.ones(rd.n_reads, dtype=bool), *sset.sel, SEED, N_LEVELS, N_REP)
    return sset


def _resident(eng, sset):
    if getattr(eng, "_rarefy_resident", None) is not sset:
        eng.upload_db(sset.species)
        eng.upload_packed(sset.reads)
        eng.rcls_profile(want_species=False)
        eng.trio_nodes_info()
        eng.get_node_abundances(fetch=False)
        eng._rarefy_resident = sset


@pytest.fixture(scope="module")
def mixed_run(eng, mixed):
    # what the seed shows, from the reference alone: among the thinned entries of a served species some are solved and some have lost every read
    thinned = [rec for per in mixed.ref[1:] for rec in per if rec["served"]]
    assert any(rec["status"] == 0 for rec in thinned) and any(rec["status"] == 1 and rec["reads"][0] == 0 for rec in thinned)
    assert any(rec["status"] == 0 and rec["n_rows"] < mixed.ref[0][s]["n_rows"] for per in mixed.ref[1:] for s, rec in enumerate(per))
    _resident(eng, mixed)
    return eng.strain_rarefy(*mixed.sel, seed=SEED, n_levels=N_LEVELS, n_replicates=N_REP)


def test_rarefy_every_entry_against_the_reference(eng, mixed, mixed_run):
    from oracle import oracle as orc
    sset = mixed
    x, obj, rows, status, reads, member = mixed_run
    sel_off, sel_hap = sset.sel
    S, E = len(sset.species), 1 + N_LEVELS * N_REP
    K = np.diff(sel_off).astype(int).tolist()
    assert K == [1, 2, 3, 64, 65, 0, 5]
    per_species = np.bincount(sset.sp[sset.sp >= 0], minlength=S)
    assert all(200 <= n <= 800 for n in per_species[:6]) and per_species[6] == 0   # a few hundred reads per species
    assert x.shape == (E, int(sel_off[-1])) and obj.shape == rows.shape == status.shape == (E, S) and reads.shape == (E, S, 2) and member.shape == (E, int(sel_off[-1]), 2)
    n_solved = n_x = n_empty = 0
    for e in range(E):
        for s in range(S):
            rec = sset.ref[e][s]
            c0, c1 = int(sel_off[s]), int(sel_off[s + 1])
            where = (e, s)
            if rec["status"] == "limit":
                assert status[e, s] == E_LIMIT and rows[e, s] == 0 and obj[e, s] == 0.0 and not x[e, c0:c1].any() and not reads[e, s].any() and not member[e, c0:c1].any(), where
                continue
            assert int(rows[e, s]) == rec["n_rows"] and int(status[e, s]) == rec["status"], where
            assert reads[e, s].tolist() == rec["reads"], (where, reads[e, s].tolist(), rec["reads"])
            assert np.array_equal(member[e, c0:c1], rec["member"]), where
            if rec["status"] == 1:
                assert obj[e, s] == 0.0 and not x[e, c0:c1].any(), where
                n_empty += int(rec["served"])
                continue
            m, a = rec["rows"]
            n, Ks = len(a), c1 - c0
            xg = x[e, c0:c1]
            assert np.all(xg >= 0.0), where
            xo, objo, _, sto = orc.lad_solve(m, a, Ks, np.full(Ks, 1.05 * a.max()))
            assert sto == 0
            assert orc.lad_objective(m, a, xg) * n == pytest.approx(obj[e, s], rel=1e-9, abs=1e-12), where
            assert obj[e, s] == pytest.approx(objo * n, rel=1e-9, abs=1e-12), (where, obj[e, s], objo * n)
            n_solved += 1
            n_x += int(np.abs(xg - xo).sum() <= 1e-9)
    assert n_solved >= 4 * N_REP * 3 and n_x >= N_REP and n_empty >= 4           # the solved LPs, the compared solutions, the entries that lost every read
    assert np.all(status[:, 4] == E_LIMIT) and np.all(status[:, 5] == 1) and np.all(status[:, 6] == 1) and not reads[:, 5:].any()
    # the levels of a replicate are nested: reads and bases never grow down the levels
    for b in range(1, N_REP + 1):
        es = [0] + [ref.entry(N_LEVELS, b, l) for l in range(1, N_LEVELS + 1)]
        assert np.all(np.diff(reads[es, :, 0].astype(np.int64), axis=0) <= 0) and np.all(np.diff(reads[es, :, 1].astype(np.int64), axis=0) <= 0)
    # entry 0 is the bootstrap's plain refit, bit for bit
    bx, bobj, brows, bstatus = eng.strain_bootstrap(*sset.sel, np.arange(S), seed=7, n_replicates=0)
    _same([x[:1], obj[:1], rows[:1], status[:1]], [bx, bobj, brows, bstatus])


# ---- 3. determinism, bit for bit

def test_rarefy_passes_route_and_position_same_bits(eng, mixed, mixed_run, set_opt):
    sset = mixed
    _resident(eng, sset)
    for cap in (1, 2, 0):                                                     # a level a pass, two, all of them
        set_opt(eng, "rarefy_levels_max", cap)
        _same(eng.strain_rarefy(*sset.sel, seed=SEED, n_levels=N_LEVELS, n_replicates=N_REP), mixed_run)
    set_opt(eng, "rarefy_levels_max", None)
    set_opt(eng, "rarefy_route", "walk")
    _same(eng.strain_rarefy(*sset.sel, seed=SEED, n_levels=N_LEVELS, n_replicates=N_REP), mixed_run)
    set_opt(eng, "rarefy_route", None)
    set_opt(eng, "rarefy_levels_max", 5)                                      # passes of 5, 5 and 2 levels
    _same(eng.strain_rarefy(*sset.sel, seed=SEED, n_levels=N_LEVELS, n_replicates=N_REP), mixed_run)
    set_opt(eng, "rarefy_levels_max", None)
    # fewer levels and replicates: the entries they share are the same (a read's depth knows neither count)
    x, obj, rows, status, reads, member = mixed_run
    few = eng.strain_rarefy(*sset.sel, seed=SEED, n_levels=2, n_replicates=2)
    pick = [0] + [ref.entry(N_LEVELS, b, l) for b in (1, 2) for l in (1, 2)]
    _same(few, [a[pick] for a in mixed_run])
    other = eng.strain_rarefy(*sset.sel, seed=SEED + 1, n_levels=2, n_replicates=2)      # another seed thins other reads; entry 0 does not know it
    _same([a[:1] for a in other], [a[:1] for a in few])
    assert not np.array_equal(other[4][1:], few[4][1:])
    # the species list reversed: every species at another position, its ids moved so that the ranges still ascend; the reads keep their order
    import synthdata as synth
    S = len(sset.species)
    rev, start, delta = [], 1, np.zeros(S, dtype=np.int64)
    for s in range(S - 1, -1, -1):
        g = sset.species[s]
        delta[s] = start - g.range_start
        rev.append(dataclasses.replace(g, range_start=start, range_end=start + g.n_nodes - 1))
        start += g.n_nodes
    rd = sset.reads
    assert np.all(sset.sp >= 0)
    step_sp = np.repeat(sset.sp, np.diff(rd.step_off.astype(np.int64)))
    rd2 = dataclasses.replace(rd, node_id=(rd.node_id.astype(np.int64) + delta[step_sp]).astype(np.uint32))
    sel_off, sel_hap = sset.sel
    off2, hap2 = _selection(rev, lambda s, H: sel_hap[int(sel_off[S - 1 - s]):int(sel_off[S - s])].tolist())
    two = synth.SyntheticSet(rev, rd2)
    _resident(eng, two)
    x2, obj2, rows2, status2, reads2, member2 = eng.strain_rarefy(off2, hap2, seed=SEED, n_levels=N_LEVELS, n_replicates=N_REP)
    for s in range(S):
        t = S - 1 - s
        c0, c1, d0, d1 = int(sel_off[s]), int(sel_off[s + 1]), int(off2[t]), int(off2[t + 1])
        assert x2[:, d0:d1].tobytes() == x[:, c0:c1].tobytes() and member2[:, d0:d1].tobytes() == member[:, c0:c1].tobytes(), s
        assert obj2[:, t].tobytes() == obj[:, s].tobytes() and np.array_equal(rows2[:, t], rows[:, s]) and np.array_equal(status2[:, t], status[:, s]), s
        assert np.array_equal(reads2[:, t], reads[:, s]), s


# ---- 4. state and arguments

def _raw(eng, sel_off, sel_hap, n_levels=2, n_replicates=2, n_species=None, fill=77):
    from pantax_amd import _ffi
    so, sh = np.ascontiguousarray(sel_off, dtype=np.uint64), np.ascontiguousarray(sel_hap, dtype=np.uint32)
    cs = _ffi.RarefySet(eng.S if n_species is None else n_species, so.ctypes.data, sh.ctypes.data if len(sh) else None, SEED, n_levels, n_replicates)
    E = 1 + 16 * max(n_replicates, 1)
    out = (np.full((E, max(len(sh), 1)), float(fill)), np.full((E, eng.S), float(fill)), np.full((E, eng.S), fill, dtype=np.uint64),
           np.full((E, eng.S), fill, dtype=np.int32), np.full((E, eng.S, 2), fill, dtype=np.uint64), np.full((E, max(len(sh), 1), 2), fill, dtype=np.uint64))
    rc = eng.lib.pantax_hip_strain_rarefy(eng.ctx, eng.db, eng.reads, C.byref(cs), *[_ffi.p(a) for a in out])
    return rc, out


def _untouched(out, fill=77):
    return all(np.all(a == fill) for a in out)


def test_rarefy_state_and_arguments(eng, mixed):
    sset = mixed
    eng._rarefy_resident = None
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    sel_off, sel_hap = sset.sel
    rc, out = _raw(eng, sel_off, sel_hap)
    assert rc == E_STATE and _untouched(out)                                   # no coverage pass yet
    bases = np.full(eng.V, 77, dtype=np.uint64)
    from pantax_amd import _ffi
    assert eng.lib.pantax_hip_rarefy_node_bases(eng.ctx, eng.db, eng.reads, SEED, 1, 1, _ffi.p(bases)) == E_STATE and np.all(bases == 77)
    eng.get_node_abundances(fetch=False)
    rc, good = _raw(eng, sel_off, sel_hap)
    assert rc == 0 and not _untouched(good)
    for kw in ({"n_levels": 0}, {"n_levels": 17}, {"n_replicates": 0}):
        rc, out = _raw(eng, sel_off, sel_hap, **kw)
        assert rc == E_INVALID and _untouched(out), kw
    twice = sel_hap.copy()
    twice[2] = twice[1]                                                        # species 1: a haplotype twice
    beyond = sel_hap.copy()
    beyond[0] = 1                                                              # species 0 has one haplotype
    for args, kw in (((sel_off, twice), {}), ((sel_off, beyond), {}), ((sel_off[:-1], sel_hap[:int(sel_off[-2])]), {"n_species": eng.S - 1})):
        rc, out = _raw(eng, *args, **kw)
        assert rc == E_INVALID and _untouched(out)
    assert eng.lib.pantax_hip_rarefy_node_bases(eng.ctx, eng.db, eng.reads, SEED, 1, 64, _ffi.p(bases)) == E_INVALID and np.all(bases == 77)
    eng.upload_packed(sset.reads)                                              # new reads, not binned against the db
    rc, out = _raw(eng, sel_off, sel_hap)
    assert rc == E_STATE and _untouched(out)
    assert eng.lib.pantax_hip_rarefy_node_bases(eng.ctx, eng.db, eng.reads, SEED, 1, 1, _ffi.p(bases)) == E_STATE and np.all(bases == 77)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    eng.get_node_abundances(fetch=False)
    rc, out = _raw(eng, sel_off, sel_hap)
    assert rc == 0
    _same(out, good)


# ---- 5. the file seam

@pytest.fixture(scope="module")
def world(tmp_path_factory):
    yield from seam_world(tmp_path_factory, "pantax_rarefy", 32, 4, 5, 30000, 30000, present_frac=0.4, single_strain_every=4, with_ids=True)


L_SEAM, B_SEAM = 3, 2


def _expected_rows(sset, db, wd, eng, n_levels, n_replicates, seed, sp_order):
    """the rows the reference builds from the stage outputs of the same sample for the rows of wd's strain_abundance.txt"""
    table = _lines(wd / "strain_abundance.txt")[1:]
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
    x, obj, rows, status, reads, member = eng.strain_rarefy(sel_off, sel_hap, seed=seed, n_levels=n_levels, n_replicates=n_replicates)
    entry_of_row = {i: (s, int(sel_off[s]) + k) for s, p in enumerate(picked) for k, (_, i) in enumerate(p)}
    exp = []
    for i, t in enumerate(table):
        s, e = entry_of_row[i]
        exp += ref.strain_rows(list(t[:3]), np.float64(t[3]), x[:, e], status[:, s], member[:, e], n_levels, n_replicates)
    for name in sp_order:
        s = names.index(name)
        exp += ref.species_rows([name], obj[:, s], status[:, s], rows[:, s], reads[:, s], n_levels, n_replicates)
    return exp, (x, status, reads)


def test_profile_seam_strain_rarefy(world, set_opt, monkeypatch):
    from pantax_amd import _ffi
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng = world
    plain, wd = root / "wd_plain", root / "wd_rf"
    _profile(eng, db, plain, gaf, strain_evidence_file=str(plain / "ev.tsv"))
    _profile(eng, db, wd, gaf, strain_evidence_file=str(wd / "ev.tsv"), strain_rarefy_file=str(wd / "rf.tsv"), strain_rarefy_levels=L_SEAM, strain_rarefy_replicates=B_SEAM)
    for f in ("species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt", "ev.tsv"):   # the option changes no table and no other report
        assert open(wd / f, "rb").read() == open(plain / f, "rb").read(), f
    assert not os.path.exists(plain / "rf.tsv")
    rows = _lines(wd / "rf.tsv")
    assert rows[0] == ref.HEADER and all(len(r) == len(ref.HEADER) for r in rows)
    rows = rows[1:]
    table = _lines(wd / "strain_abundance.txt")[1:]
    n_str = len(table) * (L_SEAM + 1)
    assert len(table) >= 2 and [tuple(r[:4]) for r in rows[:n_str:L_SEAM + 1]] == [tuple(t[:3]) + ("strain",) for t in table]
    sp_rows = rows[n_str:]
    assert all(r[1] == "-" and r[2] == "-" and r[3] == "species" for r in sp_rows)
    seq = [r[0] for r in sp_rows[::L_SEAM + 1]]
    sp_table = [r[0] for r in _lines(wd / "species_abundance.txt")[1:]]      # the run takes the selected species in the order of the species table
    assert len(set(seq)) == len(seq) >= 2 and seq == [t for t in sp_table if t in set(seq)] and {t[0] for t in table} <= set(seq)
    exp, (x, status, reads) = _expected_rows(sset, db, wd, eng, L_SEAM, B_SEAM, 42, seq)
    assert len(exp) == len(rows)
    for got, want in zip(rows, exp):
        assert ref.parse_row(got) == want, (got, want)
    assert np.all(status[0][[[g.name for g in sset.species].index(t[0]) for t in table]] == 0) and reads[1:, :, 0].sum() < B_SEAM * L_SEAM * reads[0, :, 0].sum()
    full = open(wd / "rf.tsv", "rb").read()
    # the same file from a run cut into three groups of species
    wg = root / "wd_rf_groups"
    set_opt(eng, "db_groups", 3)
    _profile(eng, db, wg, gaf, strain_rarefy_file=str(wg / "rf.tsv"), strain_rarefy_levels=L_SEAM, strain_rarefy_replicates=B_SEAM)
    set_opt(eng, "db_groups", None)
    assert open(wg / "rf.tsv", "rb").read() == full
    # the command-line front end; its defaults: 5 levels, 5 replicates, seed 42
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_rf_cli"
    wc.mkdir()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0",
                        "--strain-rarefy", str(wc / "rf.tsv"), "--strain-rarefy-levels", str(L_SEAM), "--strain-rarefy-replicates", str(B_SEAM), "--strain-rarefy-seed", "42"],
                       cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc / "rf.tsv", "rb").read() == full
    wdft = root / "wd_rf_default"
    _profile(eng, db, wdft, gaf, strain_rarefy_file=str(wdft / "rf.tsv"))
    dflt = _lines(wdft / "rf.tsv")[1:]
    assert len(dflt) == (len(table) + len(seq)) * 6 and [r[4] for r in dflt[:6]] == ["0", "1", "2", "3", "4", "5"]
    assert [r for r in dflt if r[4] == "0"] == [r for r in rows if r[4] == "0"]          # level 0 knows neither count
    # another seed: other subsamples, the same level 0; a seed of 0 passed explicitly is 0
    ws = root / "wd_rf_seed"
    _profile(eng, db, ws, gaf, strain_rarefy_file=str(ws / "rf.tsv"), strain_rarefy_levels=L_SEAM, strain_rarefy_replicates=B_SEAM, strain_rarefy_seed=0)
    other = _lines(ws / "rf.tsv")[1:]
    assert [r for r in other if r[4] == "0"] == [r for r in rows if r[4] == "0"] and other != rows
    exp0, _ = _expected_rows(sset, db, ws, eng, L_SEAM, B_SEAM, 0, seq)
    assert [ref.parse_row(r) for r in other] == exp0
    # several ranks: refused on every rank with the table's wording, before any collective
    for rank in range(2):
        wn = root / ("wd_rf_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, strain_rarefy_file=str(wn / "rf.tsv"))
        assert e.value.code == E_INVALID and "the rarefaction report (strain_rarefy_file) needs one rank and an unsharded ingest (world_size 2)" in str(e.value)
        assert not os.path.exists(wn / "rf.tsv")
    with pytest.raises(PantaxHipError) as e:
        _profile(eng, db, root / "wd_rf_17", gaf, strain_rarefy_file=str(root / "wd_rf_17" / "rf.tsv"), strain_rarefy_levels=17)
    assert e.value.code == E_INVALID and "strain_rarefy_levels 17" in str(e.value)
    # a caller compiled against the header before these fields: its struct ends behind strain_links_top, the report reads as off
    real = _ffi.ProfileExt

    class OldExt(real):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.struct_size = 168

    monkeypatch.setattr(_ffi, "ProfileExt", OldExt)
    wold = root / "wd_rf_old"
    _profile(eng, db, wold, gaf, strain_fit_file=str(wold / "fit.tsv"), strain_rarefy_file=str(wold / "rf.tsv"))
    monkeypatch.setattr(_ffi, "ProfileExt", real)
    assert os.path.exists(wold / "fit.tsv") and not os.path.exists(wold / "rf.tsv")
    assert open(wold / "strain_abundance.txt", "rb").read() == open(wd / "strain_abundance.txt", "rb").read()
