"""GPU tests of the add-one test of the strain fit (pantax_hip_strain_addin, --strain-addin).  The rows of every species come from the numpy restatement
of the contract in tests/bootstrap_ref.py, applied over the columns Sel ++ Cand to the bases_per_node that get_node_abundances hands out; the reference of
every entry is the oracle's own solver with the pinned candidates' upper bounds at zero (tests/addin_ref.py, checked against SciPy-HiGHS in
tests/test_addin_ref.py).  Per entry: status and rows exact, the objective of the device's x equal to obj_out and both equal to the oracle's optimum to the
project's LP tolerance (rel 1e-9, abs 1e-12); x itself is compared through the objective only (LAD optima are not unique); the four counts equal the numpy
recount from the delivered x, exactly.  Everything that must not depend on the chunking, the route or the position of the species is compared bit for bit."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile
from tests import addin_ref as ref
from tests import dropout_ref

pytestmark = pytest.mark.gpu

E_INVALID, E_LIMIT, E_SOLVER, E_STATE = -1, -4, -5, -7


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _coverage(eng, sset):
    """the set resident with a coverage result of the stage kind -> bases_per_node; computed once per set"""
    if getattr(eng, "_addin_resident", None) is not sset:
        eng.upload_db(sset.species)
        eng.upload_packed(sset.reads)
        eng.rcls_profile(want_species=False)
        eng.trio_nodes_info()
        bases, _, _, _ = eng.get_node_abundances()
        sset._addin_bases = np.array(bases, copy=True)
        eng._addin_resident = sset
    return sset._addin_bases


def _visits(g):
    v = np.zeros((g.n_nodes, g.n_paths), dtype=bool)
    for h in range(g.n_paths):
        v[g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])], h] = True
    return v


def _sets(species, pick):
    """pick(s, H) -> (reported, candidates) of species s -> (sel_off, sel_hap, cand_off, cand_hap)"""
    so, sh, co, ch = [0], [], [0], []
    for s, g in enumerate(species):
        rep, cand = pick(s, g.n_paths)
        sh.extend(rep)
        ch.extend(cand)
        so.append(len(sh))
        co.append(len(ch))
    return np.array(so, dtype=np.uint64), np.array(sh, dtype=np.uint32), np.array(co, dtype=np.uint64), np.array(ch, dtype=np.uint32)


def _custom(name, node_len, paths, start, depth):
    """a species graph from explicit walks"""
    import synthdata as synth
    node_len = np.asarray(node_len, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.uint64)
    nodes = np.concatenate(paths).astype(np.uint32)
    glen = np.array([int(node_len[np.asarray(p)].sum()) for p in paths], dtype=np.int64)
    return synth.SpeciesGraph(name, node_len, off, nodes, ["GCF_%s_%03d" % (name, h) for h in range(len(paths))], start, start + len(node_len) - 1, glen,
                              np.asarray(depth, dtype=np.float64))


def _reference(sset, bases, sets):
    """tests/addin_ref.py over every species: computed once per set and left unchanged"""
    sel_off, sel_hap, cand_off, cand_hap = sets
    node_off = np.concatenate([[0], np.cumsum([g.n_nodes for g in sset.species])])
    out = []
    for s, g in enumerate(sset.species):
        cols = np.concatenate([sel_hap[int(sel_off[s]):int(sel_off[s + 1])], cand_hap[int(cand_off[s]):int(cand_off[s + 1])]]).astype(np.int64)
        member = _visits(g)[:, cols] if len(cols) else np.zeros((g.n_nodes, 0), dtype=bool)
        out.append(ref.species_addin(g.node_len, bases[node_off[s]:node_off[s + 1]], member, int(sel_off[s + 1]) - int(sel_off[s])))
    return out


def _check_against_reference(refs, sets, got, refit=None):
    """every entry of `got` against the reference; refit: the objective of pantax_hip_strain_dropout's entry 0 on Sel alone, per species (None where it
    has none) -> entries checked"""
    from oracle import oracle as orc
    from pantax_amd.engine import addin_donor
    sel_off, _, cand_off, _ = sets
    x, obj, status, rows, count = got
    S = len(refs)
    Q = int(cand_off[-1]) + S
    assert len(x) == S and obj.shape == status.shape == (Q,) and rows.shape == (S,) and count.shape == (Q, 4)
    n_checked = 0
    for s, d in enumerate(refs):
        K, J = int(sel_off[s + 1]) - int(sel_off[s]), int(cand_off[s + 1]) - int(cand_off[s])
        W, E = K + J, J + 1
        q0 = ref.entry(cand_off, s, 0)
        assert x[s].shape == (E, W)
        assert int(rows[s]) == d["rows"], s
        assert status[q0:q0 + E].tolist() == d["status"].tolist(), (s, status[q0:q0 + E], d["status"])
        if W > 64 or W == 0 or d["rows"] == 0:
            assert not x[s].any() and not obj[q0:q0 + E].any() and not count[q0:q0 + E].any()
            continue
        mask, a = d["mask"], d["a"]
        assert count[q0].tolist() == ref.counts0(mask, K).tolist(), s
        a_novel = a[ref.no_reported_bit(mask, K)].sum()
        for e in range(E):
            q = q0 + e
            xg = x[s][e]
            assert np.all(xg >= 0.0) and np.all(xg <= 1.05 * a.max()), (s, e)
            at_x = orc.lad_objective(mask, a, xg) * len(a) if xg.any() else float(a.sum())
            print("species %d (K %d, J %d) entry %d: obj %.17g, objective at x %.17g, oracle %.17g" % (s, K, J, e, obj[q], at_x, d["obj"][e]))
            assert at_x == pytest.approx(obj[q], rel=1e-9, abs=1e-12), (s, e)
            assert obj[q] == pytest.approx(d["obj"][e], rel=1e-9, abs=1e-12), (s, e, obj[q], d["obj"][e])
            pinned = [K + c for c in range(J) if c + 1 != e]
            assert not xg[pinned].any() and not np.signbit(xg[pinned]).any(), (s, e)
            if e == 0:
                if K == 0:
                    assert obj[q] == pytest.approx(a.sum(), rel=1e-12) and not xg.any(), s
                if refit is not None and refit[s] is not None:
                    print("species %d: entry 0 %.17g, the refit on Sel alone %.17g + %.17g on the rows without a reported bit" % (s, obj[q], refit[s], a_novel))
                    assert obj[q] <= (refit[s] + a_novel) * (1 + 1e-9), s
            else:
                c = e - 1
                assert obj[q] <= obj[q0] * (1 + 1e-9), (s, e)
                assert count[q].tolist() == ref.counts(mask, a, K, x[s][0], xg, c).tolist(), (s, e)
                assert addin_donor(K, x[s][0], xg) == ref.donor(K, x[s][0], xg), (s, e)
            n_checked += 1
    return n_checked


def _flat(got):
    x, obj, status, rows, count = got
    return [np.concatenate([b.ravel() for b in x]) if len(x) else np.zeros(0), obj, status, rows, count]


def _same(a, b):
    for p, q in zip(_flat(a), _flat(b)):
        assert p.dtype == q.dtype and p.shape == q.shape and p.tobytes() == q.tobytes()


# ---- (K_s, J_s) over every instance of the solver and of the objective pass, the limit, no candidate, no column, no read; chunks of one round, two and all;
# both routes

KJ = [(1, 1), (2, 5), (3, 5), (16, 16), (32, 32), (1, 63), (0, 64), (60, 5), (4, 0), (0, 0), (2, 2)]


@pytest.fixture(scope="module")
def mixed():
    import synthdata as synth
    rng = np.random.default_rng(951)
    species, start = [], 1
    for s, (K, J) in enumerate(KJ):
        h = max(K + J, 3)
        g = synth.make_species(rng, str(3000 + s), h, 8000 if h < 64 else 4000, start, "GCF_%06d" % (s + 1), present_frac=0.5)
        if s == len(KJ) - 1:
            g.truth_depth[:] = 0.0                                           # no read of this species: no covered node
        species.append(g)
        start = g.range_end + 1
    sset = synth.SyntheticSet(species, synth.make_reads(rng, species, 6000))
    shuffle = np.random.default_rng(7)

    def pick(s, H):   # Sel and Cand in a shuffled order (column = position in the lists, not haplotype index)
        order = [int(h) for h in shuffle.permutation(H)]
        return order[:KJ[s][0]], order[KJ[s][0]:KJ[s][0] + KJ[s][1]]
    sset.sets = _sets(species, pick)
    return sset


@pytest.fixture(scope="module")
def mixed_run(eng, mixed):
    bases = _coverage(eng, mixed)
    return bases, eng.strain_addin(*mixed.sets), _reference(mixed, bases, mixed.sets)


def test_addin_every_entry_against_the_oracle(eng, mixed, mixed_run):
    sset = mixed
    bases, got, refs = mixed_run
    sel_off, sel_hap, cand_off, cand_hap = sset.sets
    assert list(zip(np.diff(sel_off).astype(int).tolist(), np.diff(cand_off).astype(int).tolist())) == KJ
    assert all(200 <= g.n_nodes <= 2000 for g in sset.species)
    x, obj, status, rows, count = got
    # the refit of the leave-one-out call on Sel alone: its rows are those with a reported bit, its box the smaller one
    dx, dobj, dstatus, _, _ = eng.strain_dropout(sel_off, sel_hap)
    refit = [float(dobj[dropout_ref.entry(sel_off, s, 0)]) if dstatus[dropout_ref.entry(sel_off, s, 0)] == 0 else (0.0 if KJ[s][0] == 0 else None) for s in range(len(KJ))]
    n_checked = _check_against_reference(refs, sset.sets, got, refit)
    assert n_checked == sum(J + 1 for K, J in KJ[:7]) + 1                     # the seven covered species with candidates, every entry, and the one entry of (4, 0)
    q = [ref.entry(cand_off, s, 0) for s in range(len(KJ))]
    assert np.all(status[q[7]:q[7] + 6] == E_LIMIT) and rows[7] == 0 and rows[8] > 0 and status[q[8]] == 0   # 65 columns; the species beside it is served
    assert status[q[9]] == 1 and np.all(status[q[10]:q[10] + 3] == 1) and rows[9] == 0 and rows[10] == 0
    # K_s = 0: entry 0 is all-pinned, solved by nobody, and costs every row
    assert status[q[6]] == 0 and not x[6][0].any() and obj[q[6]] == pytest.approx(refs[6]["a"].sum(), rel=1e-12) and count[q[6]].tolist() == [rows[6], rows[6], 0, 0]
    # half of every species' haplotypes have reads, so some dropped candidate improves the fit and moves rows both ways
    assert any(obj[q[s] + e] < 0.99 * obj[q[s]] for s in range(1, 7) for e in range(1, KJ[s][1] + 1))
    assert count[:, 2].max() > 0 and count[:, 3].max() > 0 and count[:, 1].max() > 0


def test_addin_chunks_routes_same_bits(eng, mixed, mixed_run, set_opt):
    sset = mixed
    bases, got, refs = mixed_run
    sel_off, sel_hap, cand_off, cand_hap = sset.sets
    P = sum(len(np.unique(d["mask"])) for d in refs)                           # the base patterns: runs of equal (species, mask)
    for cap in (P + 1, 2 * (P + 1), 3 * (P + 1) - 1, 65 * (P + 1)):            # one round a chunk; two; two again; all 65 rounds
        set_opt(eng, "addin_patterns_max", cap)
        _same(eng.strain_addin(*sset.sets), got)
    set_opt(eng, "addin_patterns_max", P)                                      # not even one round: refused, the reason says so, the outputs stay
    rc, out = _raw(eng, *sset.sets)
    assert rc == E_LIMIT and _untouched(out) and "addin_patterns_max" in eng.lib.pantax_hip_last_error(eng.ctx).decode()
    set_opt(eng, "addin_patterns_max", None)
    set_opt(eng, "addin_route", "walk")
    _same(eng.strain_addin(*sset.sets), got)
    set_opt(eng, "addin_route", None)
    # two calls in a row, a call behind the bootstrap and one behind the leave-one-out test, on the same coverage result
    _same(eng.strain_addin(*sset.sets), got)
    eng.strain_bootstrap(sel_off, sel_hap, np.arange(len(sset.species), dtype=np.uint64), n_replicates=1)
    _same(eng.strain_addin(*sset.sets), got)
    eng.strain_dropout(sel_off, sel_hap)
    _same(eng.strain_addin(*sset.sets), got)
    # J = 0 everywhere: entry 0 is the bootstrap's replicate 0 on the same rows
    none = np.zeros(len(sset.species) + 1, dtype=np.uint64)
    ok = [s for s, (K, J) in enumerate(KJ) if K <= 64]
    so = np.concatenate([[0], np.cumsum([KJ[s][0] if s in ok else 0 for s in range(len(KJ))])]).astype(np.uint64)
    sh = np.concatenate([sel_hap[int(sel_off[s]):int(sel_off[s + 1])] for s in ok]).astype(np.uint32)
    plain = eng.strain_addin(so, sh, none, np.zeros(0, dtype=np.uint32))
    xb, objb, rowsb, stb = eng.strain_bootstrap(so, sh, np.arange(len(sset.species), dtype=np.uint64), n_replicates=0)
    assert np.array_equal(rowsb[0], plain[3]) and np.array_equal(stb[0], plain[2])
    for s in range(len(sset.species)):
        assert objb[0, s] == pytest.approx(plain[1][s], rel=1e-9, abs=1e-12)


# ---- crafted graphs (tests/addin_ref.py CRAFTED): a candidate with the walk of a reported strain; a strain with reads and covered private nodes left out of
# Sel; no reported strain and one candidate

@pytest.fixture(scope="module")
def crafted():
    import synthdata as synth
    rng = np.random.default_rng(952)
    species, start = [], 1
    for i, name in enumerate(sorted(ref.CRAFTED)):
        case = ref.CRAFTED[name]
        species.append(_custom(str(5100 + i), np.full(case["n_nodes"], 60), case["walks"], start, case["depth"]))
        start = species[-1].range_end + 1
    sset = synth.SyntheticSet(species, synth.make_reads(rng, species, 2000, adversarial_frac=0.0))
    cases = [ref.CRAFTED[name] for name in sorted(ref.CRAFTED)]
    sset.sets = _sets(species, lambda s, H: (cases[s]["sel"], cases[s]["cand"]))
    return sset


def test_addin_crafted_graphs(eng, crafted):
    """each stated answer is asked of the reference on the device's rows first, then of the device"""
    sset = crafted
    bases = _coverage(eng, sset)
    got = eng.strain_addin(*sset.sets)
    refs = _reference(sset, bases, sset.sets)
    names = sorted(ref.CRAFTED)
    assert _check_against_reference(refs, sset.sets, got) == sum(len(ref.CRAFTED[n]["cand"]) + 1 for n in names)
    x, obj, status, rows, count = got
    for s, name in enumerate(names):
        E = len(ref.CRAFTED[name]["cand"]) + 1
        q0 = ref.entry(sset.sets[2], s, 0)
        assert int(rows[s]) == ref.CRAFTED[name]["n_nodes"], name             # every node of the crafted species is covered
        ref.assert_crafted("reference", name, refs[s])
        ref.assert_crafted("device", name, dict(a=refs[s]["a"], x=x[s], obj=obj[q0:q0 + E], count=count[q0:q0 + E]))
    # the dropped strain takes its coverage from the one reported strain
    s = names.index("dropped")
    c = ref.CRAFTED["dropped"]["cand"].index(1)
    for who, xs in (("reference", refs[s]["x"]), ("device", x[s])):
        j, loss, shift = ref.donor(1, xs[0], xs[c + 1])
        print("%s: donor %d, loss %.17g, coverage %.17g" % (who, j, loss, xs[c + 1][1 + c]))
        assert j == 0 and loss > 0 and shift == loss, who
    # one candidate alone: a one-column LP
    s = names.index("alone")
    assert x[s][1][0] == pytest.approx(np.median(refs[s]["a"]), rel=0.2)


# ---- the position of the species in the db

def test_addin_species_position(eng):
    """the same species at index 0 of one db and at index 2 of another: the same bits"""
    import synthdata as synth
    rng = np.random.default_rng(953)
    X = synth.make_species(rng, "4200", 6, 8000, 1, "GCF_X", present_frac=0.6)
    reads = synth.make_reads(rng, [X], 1500, adversarial_frac=0.0)
    A = synth.make_species(rng, "4201", 3, 6000, 1, "GCF_A", present_frac=0.5)
    B = synth.make_species(rng, "4202", 4, 6000, A.range_end + 1, "GCF_B", present_frac=0.5)
    shift = B.range_end
    X2 = dataclasses.replace(X, range_start=X.range_start + shift, range_end=X.range_end + shift)
    reads2 = dataclasses.replace(reads, node_id=(reads.node_id + np.uint32(shift)).astype(np.uint32))
    one, three = synth.SyntheticSet([X], reads), synth.SyntheticSet([A, B, X2], reads2)
    b1 = _coverage(eng, one)
    sel_x, cand_x = [3, 0, 4], [5, 1]
    r1 = eng.strain_addin([0, 3], sel_x, [0, 2], cand_x)
    b3 = _coverage(eng, three)
    assert np.array_equal(b3[-X.n_nodes:], b1) and b1.any() and not b3[:-X.n_nodes].any()
    r3 = eng.strain_addin([0, 2, 2, 5], [1, 0] + sel_x, [0, 1, 1, 3], [2] + cand_x)
    # species 2 of the second db: entries 3 .. 5 of 6 (two entries of the first species, then the one entry of the species without a column, before it)
    assert r3[0][2].tobytes() == r1[0][0].tobytes() and r3[1][3:].tobytes() == r1[1].tobytes() and r3[4][3:].tobytes() == r1[4].tobytes()
    assert np.array_equal(r3[2][3:], r1[2]) and r3[3][2] == r1[3][0] > 0 and np.all(r1[2] == 0)
    assert np.all(r3[2][:3] == 1) and r1[0][0].std(axis=0).max() > 0


# ---- state and arguments

def _raw(eng, sel_off, sel_hap, cand_off, cand_hap, n_species=None, fill=77):
    from pantax_amd import _ffi
    so, sh = np.ascontiguousarray(sel_off, dtype=np.uint64), np.ascontiguousarray(sel_hap, dtype=np.uint32)
    co, ch = np.ascontiguousarray(cand_off, dtype=np.uint64), np.ascontiguousarray(cand_hap, dtype=np.uint32)
    cs = _ffi.NearMissSet(eng.S if n_species is None else n_species, so.ctypes.data, sh.ctypes.data if len(sh) else None, co.ctypes.data, ch.ctypes.data if len(ch) else None)
    Q = len(ch) + eng.S
    n = min(len(so), len(co))
    K, J = np.diff(so.astype(np.int64))[:n - 1], np.diff(co.astype(np.int64))[:n - 1]
    x = np.full(max(int(((J + 1) * (K + J)).sum()), 1), float(fill))
    obj = np.full(Q, float(fill))
    st = np.full(Q, fill, dtype=np.int32)
    rows = np.full(eng.S, fill, dtype=np.uint64)
    cnt = np.full((Q, 4), fill, dtype=np.uint64)
    rc = eng.lib.pantax_hip_strain_addin(eng.ctx, eng.db, C.byref(cs), _ffi.p(x), _ffi.p(obj), _ffi.p(st), _ffi.p(rows), _ffi.p(cnt))
    return rc, (x, obj, st, rows, cnt)


def _untouched(out, fill=77):
    return all(np.all(a == fill) for a in out)


def test_addin_state_and_arguments(eng, mixed, set_opt):
    from pantax_amd._ffi import PantaxHipError
    sset = mixed
    eng._addin_resident = None
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    sel_off, sel_hap, cand_off, cand_hap = sset.sets
    rc, out = _raw(eng, *sset.sets)
    assert rc == E_STATE and _untouched(out)                                   # no coverage pass yet
    eng.get_node_abundances(fetch=False)
    rc, out = _raw(eng, *sset.sets)
    assert rc == 0 and not _untouched(out)
    good = out
    s1, c1 = int(sel_off[1]), int(cand_off[1])                                 # species 1: two reported, five candidates
    sel_twice, cand_twice, both, beyond = sel_hap.copy(), cand_hap.copy(), cand_hap.copy(), cand_hap.copy()
    sel_twice[s1 + 1] = sel_twice[s1]                                          # a haplotype twice within Sel_s
    cand_twice[c1 + 1] = cand_twice[c1]                                        # ... twice within Cand_s
    both[c1] = sel_hap[s1]                                                     # ... in both
    beyond[c1] = sset.species[1].n_paths                                       # ... out of range
    for args, kw in (((sel_off, sel_twice, cand_off, cand_hap), {}), ((sel_off, sel_hap, cand_off, cand_twice), {}), ((sel_off, sel_hap, cand_off, both), {}),
                     ((sel_off, sel_hap, cand_off, beyond), {}),
                     ((sel_off[:-1], sel_hap[:int(sel_off[-2])], cand_off[:-1], cand_hap[:int(cand_off[-2])]), {"n_species": eng.S - 1})):
        rc, out = _raw(eng, *args, **kw)
        assert rc == E_INVALID and _untouched(out)
    set_opt(eng, "addin_patterns_max", 1)                                      # a limit of the call's own: the outputs are left as given
    rc, out = _raw(eng, *sset.sets)
    assert rc == E_LIMIT and _untouched(out)
    set_opt(eng, "addin_patterns_max", None)
    eng.profile_step(sset.avg_len())                                           # a resident step may zero the arena
    with pytest.raises(PantaxHipError) as e:
        eng.strain_addin(*sset.sets)
    assert e.value.code == E_STATE and "resident step" in str(e.value)
    rc, out = _raw(eng, *sset.sets)
    assert rc == E_STATE and _untouched(out)
    eng.get_node_abundances(fetch=False)
    rc, out = _raw(eng, *sset.sets)
    assert rc == 0 and all(p.tobytes() == q.tobytes() for p, q in zip(out, good))


# ---- the file seam -----------------------------------------------------------------------------------------------------------

HEADER = ["species_taxid", "strain_taxid", "genome_ID", "rank", "class", "n_rows", "objective", "objective_with", "gain", "gain_fraction", "coverage", "n_member", "n_novel",
          "n_better", "n_worse", "donor_strain_taxid", "donor_genome_ID", "donor_loss", "shift", "stage", "unique_trio_nodes_fraction"]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from tests.helpers import seam_world
    yield from seam_world(tmp_path_factory, "pantax_addin", 32, 4, 5, 30000, 30000, present_frac=0.4, single_strain_every=4, with_ids=True)


def _stage_resident(eng, sset):
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    eng.get_node_abundances(fetch=False)


def _f(x):
    return np.float64(x)


def _expected_rows(sset, db, wd, eng, top):
    """the report from the stage calls and the run's tables: Sel = the rows of strain_abundance.txt in ascending haplotype index, Cand = every other
    haplotype (the world's species are narrow) scored by Engine.strain_near_miss, ranked by near_miss_rank and cut to 64 - K; every cell from one
    Engine.strain_addin call over them"""
    from pantax_amd.engine import addin_donor, near_miss_rank
    table = _lines(wd / "strain_abundance.txt")[1:]
    ori = {(r[0], r[2]): r for r in _lines(wd / "ori_strain_abundance.txt")[1:]}
    names = [g.name for g in sset.species]
    genomes = _lines(db / "genomes_info.txt")[1:]
    col = {c: i for i, c in enumerate(_lines(db / "genomes_info.txt")[0])}
    genome_of = {}
    for r in genomes:
        genome_of.setdefault(r[0].split("_ASM")[0], r)                       # the first row of every haplotype
    hap_of_genome = {r[0]: r[0].split("_ASM")[0] for r in genomes}
    reported = [set() for _ in names]
    for t in table:
        s = names.index(t[0])
        reported[s].add(sset.species[s].hap_names.index(hap_of_genome[t[2]]))
    all_sets = _sets(sset.species, lambda s, H: (sorted(reported[s]), [h for h in range(H) if h not in reported[s]]))
    cand, _ = eng.strain_near_miss(*all_sets)
    tested = []
    for s in range(len(names)):
        c0, c1 = int(all_sets[2][s]), int(all_sets[2][s + 1])
        order = near_miss_rank(all_sets[3][c0:c1], cand[c0:c1], top) if c1 > c0 else []
        tested.append([int(all_sets[3][c0 + c]) for c in order][:max(0, 64 - len(reported[s]))])
    sets = _sets(sset.species, lambda s, H: (sorted(reported[s]), tested[s]))
    x, obj, status, nrows, count = eng.strain_addin(*sets)
    seq = [r[0] for r in _lines(wd / "ev.tsv")[1:] if r[3] == "total"]       # the species that went through the strain step, in the run's order
    assert len(set(seq)) == len(seq) >= 2 and {t[0] for t in table} <= set(seq)
    rows = []
    for sp in seq:
        s = names.index(sp)
        K, q0 = len(reported[s]), ref.entry(sets[2], s, 0)
        sel = sorted(reported[s])
        for c, h in enumerate(tested[s]):
            g = genome_of.get(sset.species[s].hap_names[h])
            o = ori.get((sp, g[0] if g else ""))
            assert o is not None, "a tested candidate of a species without rows in ori_strain_abundance.txt"
            stage = "first_filter" if o[8] == "" else ("second_filter" if o[3] == "" else "table_filter")
            head = [sp, g[col["strain_taxid"]] if g else "", g[0] if g else "", str(c + 1), "candidate"]
            assert status[q0] == 0 and status[q0 + 1 + c] == 0
            gain = obj[q0] - obj[q0 + 1 + c]
            cells = [str(int(nrows[s])), _f(obj[q0]), _f(obj[q0 + 1 + c]), _f(gain), _f(gain / obj[q0]) if obj[q0] != 0 else "-", _f(x[s][c + 1][K + c])]
            cells += [str(int(v)) for v in count[q0 + 1 + c]]
            j, loss, shift = addin_donor(K, x[s][0], x[s][c + 1])
            dg = genome_of.get(sset.species[s].hap_names[sel[j]]) if j >= 0 else None
            cells += ["-", "-", "-"] if j < 0 else [dg[col["strain_taxid"]] if dg else "", dg[0] if dg else "", _f(loss)]
            cells += [_f(shift), stage, _f(o[6]) if o[6] else "-"]
            rows.append(head + cells)
    for sp in seq:
        s = names.index(sp)
        if not reported[s] and not tested[s]:
            continue
        q0 = ref.entry(sets[2], s, 0)
        rows.append([sp, "-", "-", "-", "species", str(int(nrows[s])), _f(obj[q0])] + ["-"] * 5 + [str(int(count[q0][1]))] + ["-"] * 8)
    return rows, tested


def _same_rows(got, exp):
    assert len(got) == len(exp), (len(got), len(exp))
    for a, b in zip(got, exp):
        assert len(a) == len(b) == len(HEADER), (a, b)
        for p, q in zip(a, b):
            if isinstance(q, np.float64):
                assert np.float64(p) == q, (a, b)
            else:
                assert p == q, (a, b)


def test_profile_seam_strain_addin(world, set_opt, monkeypatch):
    from pantax_amd import _ffi
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng = world
    # a min_cov between the predicted coverages of the table drops its weakest rows at the a15 filter: strains that are in the sample and no longer in the
    # table, the case the report is for (the cut of test_profile_seam_strain_near_miss)
    _profile(eng, db, root / "wd_all", gaf)
    covs = sorted(float(r[3]) for r in _lines(root / "wd_all" / "strain_abundance.txt")[1:])
    cuts = [int(c) + 1 for c in covs if sum(v < int(c) + 1 for v in covs) >= 1 and sum(v >= int(c) + 1 for v in covs) >= 2]
    assert cuts, covs
    mc = cuts[0]
    plain, wd = root / "wd_plain", root / "wd_addin"
    set_opt(eng, "db_groups", 1)
    _profile(eng, db, plain, gaf, min_cov=mc)
    _profile(eng, db, wd, gaf, min_cov=mc, strain_addin_file=str(wd / "addin.tsv"), strain_evidence_file=str(wd / "ev.tsv"))
    for f in ("species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt"):   # the option changes none of the tables
        assert open(wd / f, "rb").read() == open(plain / f, "rb").read()
    assert not os.path.exists(plain / "addin.tsv")
    rows = _lines(wd / "addin.tsv")
    assert rows[0] == HEADER and all(len(r) == len(HEADER) for r in rows)
    # every cell from a stage call of the same sample whose candidates are rebuilt with Engine.strain_near_miss and near_miss_rank
    _stage_resident(eng, sset)
    exp, tested = _expected_rows(sset, db, wd, eng, 5)                         # top 0 = the default of 5
    _same_rows(rows[1:], exp)
    n_cand = sum(len(t) for t in tested)
    assert n_cand >= 1 and [r[4] for r in rows[1:1 + n_cand]] == ["candidate"] * n_cand and all(r[4] == "species" and r[1:4] == ["-"] * 3 for r in rows[1 + n_cand:])
    assert len(rows) - 1 - n_cand >= 2
    assert any(float(r[8]) > 0 and float(r[10]) > 0 and int(r[12]) > 0 and r[19] == "table_filter" for r in rows[1:1 + n_cand])   # a dropped strain the sample wants back
    assert any(r[15] != "-" for r in rows[1:1 + n_cand])
    # the same file from a run cut into three groups of species, and from one cut by the path steps a resident db may hold
    wg = root / "wd_addin_groups"
    set_opt(eng, "db_groups", 3)
    _profile(eng, db, wg, gaf, min_cov=mc, strain_addin_file=str(wg / "addin.tsv"))
    set_opt(eng, "db_groups", None)
    assert open(wg / "addin.tsv", "rb").read() == open(wd / "addin.tsv", "rb").read()
    ws = root / "wd_addin_steps"
    set_opt(eng, "db_path_steps_max", int(max(len(g.path_nodes) for g in sset.species) * 3))
    _profile(eng, db, ws, gaf, min_cov=mc, strain_addin_file=str(ws / "addin.tsv"))
    set_opt(eng, "db_path_steps_max", None)
    assert open(ws / "addin.tsv", "rb").read() == open(wd / "addin.tsv", "rb").read()
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_addin_cli"
    wc.mkdir()
    run = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0", "--min_cov", str(mc),
                          "--strain-addin", str(wc / "addin.tsv"), "--strain-addin-top", "5"], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert open(wc / "addin.tsv", "rb").read() == open(wd / "addin.tsv", "rb").read()
    # beside the near-miss report, the leave-one-out test and the bootstrap: the same bytes, and theirs as without it
    wb, wo = root / "wd_addin_all", root / "wd_addin_others"
    others = lambda w: dict(strain_near_miss_file=str(w / "nm.tsv"), strain_dropout_file=str(w / "drop.tsv"), strain_bootstrap_file=str(w / "boot.tsv"), strain_bootstrap_replicates=2)
    _profile(eng, db, wb, gaf, min_cov=mc, strain_addin_file=str(wb / "addin.tsv"), **others(wb))
    _profile(eng, db, wo, gaf, min_cov=mc, **others(wo))
    assert open(wb / "addin.tsv", "rb").read() == open(wd / "addin.tsv", "rb").read()
    for f in ("nm.tsv", "drop.tsv", "boot.tsv"):
        assert open(wb / f, "rb").read() == open(wo / f, "rb").read(), f
    # --strain-addin-top 1: one candidate a species
    wt = root / "wd_addin_top1"
    _profile(eng, db, wt, gaf, min_cov=mc, strain_addin_file=str(wt / "addin.tsv"), strain_addin_top=1, strain_evidence_file=str(wt / "ev.tsv"))
    _stage_resident(eng, sset)
    exp1, tested1 = _expected_rows(sset, db, wt, eng, 1)
    _same_rows(_lines(wt / "addin.tsv")[1:], exp1)
    assert all(len(t) <= 1 for t in tested1) and [t[:1] for t in tested] == tested1 and all(r[3] == "1" for r in _lines(wt / "addin.tsv")[1:] if r[4] == "candidate")
    # several ranks: refused with the plan's wording, nothing written
    for rank in range(2):
        wn = root / ("wd_addin_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, strain_addin_file=str(wn / "addin.tsv"))
        assert e.value.code == E_INVALID and "the add-one report (strain_addin_file) needs one rank and an unsharded ingest (world_size 2)" in str(e.value)
        assert not os.path.exists(wn / "addin.tsv") and not os.path.exists(wn / "species_abundance.txt")
    # a caller compiled against the header before these fields: its struct ends behind strain_dropout_file, the report reads as off
    real = _ffi.ProfileExt

    class OldExt(real):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.struct_size = 48

    monkeypatch.setattr(_ffi, "ProfileExt", OldExt)
    wold = root / "wd_addin_old"
    _profile(eng, db, wold, gaf, min_cov=mc, strain_dropout_file=str(wold / "drop.tsv"), strain_addin_file=str(wold / "addin.tsv"))
    monkeypatch.setattr(_ffi, "ProfileExt", real)
    assert os.path.exists(wold / "drop.tsv") and not os.path.exists(wold / "addin.tsv")
    assert open(wold / "drop.tsv", "rb").read() == open(wo / "drop.tsv", "rb").read()
    assert open(wold / "strain_abundance.txt", "rb").read() == open(wd / "strain_abundance.txt", "rb").read()


def test_profile_seam_addin_skips_a_species_of_65_rows(tmp_path_factory):
    """a species with more rows in strain_abundance.txt than the call serves prints `skipped`; the species beside it is served (the inputs of
    test_profile_seam_dropout_skips_a_species_of_65_rows)"""
    import synthdata as synth
    from pantax_amd.engine import Engine
    rng = np.random.default_rng(944)
    wide = synth.make_species(rng, "7000", 100, 30000, 1, "GCF_W", present_frac=1.0)
    small = synth.make_species(rng, "7001", 3, 8000, wide.range_end + 1, "GCF_S", present_frac=1.0)
    sset = synth.SyntheticSet([wide, small], synth.make_reads(rng, [wide, small], 60000, adversarial_frac=0.0, with_ids=True))
    root = tmp_path_factory.mktemp("pantax_addin_wide")
    db = root / "db"
    db.mkdir()
    synth.write_db(sset, str(db))
    gaf = root / "gfa_mapped.gaf"
    synth.write_gaf(sset.reads, str(gaf))
    eng = Engine(0)
    try:
        wd = root / "wd"
        _profile(eng, db, wd, gaf, fr=0.0, fc=1e9, sd=1e9, strain_addin_file=str(wd / "addin.tsv"))
    finally:
        eng.close()
    table = _lines(wd / "strain_abundance.txt")[1:]
    n_wide = sum(1 for t in table if t[0] == "7000")
    print("rows of the wide species in the strain table: %d" % n_wide)
    assert n_wide >= 65
    rows = _lines(wd / "addin.tsv")
    assert rows[0] == HEADER and all(len(r) == len(HEADER) for r in rows)
    assert not any(r[0] == "7000" and r[4] == "candidate" for r in rows[1:])
    by = {r[0]: r for r in rows[1:] if r[4] != "candidate"}
    assert by["7000"][4] == "skipped" and by["7000"][6] == "-" and by["7000"][12] == "-"
    assert by["7001"][4] == "species" and int(by["7001"][5]) > 0 and float(by["7001"][6]) >= 0 and int(by["7001"][12]) >= 0
