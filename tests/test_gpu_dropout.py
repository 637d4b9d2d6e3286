"""GPU tests of the leave-one-out test of the strain fit (pantax_hip_strain_dropout, --strain-dropout).  The rows of every species come from the numpy
restatement of the contract in tests/bootstrap_ref.py, applied to the bases_per_node that get_node_abundances hands out; the reference of every entry is
the oracle's own solver with the dropped column's upper bound at zero (tests/dropout_ref.py, checked against SciPy-HiGHS in tests/test_dropout_ref.py).
Per entry: status and rows exact, the objective of the device's x equal to obj_out and both equal to the oracle's optimum to the project's LP tolerance
(rel 1e-9, abs 1e-12); x itself is compared through the objective only (LAD optima are not unique); the four counts equal the numpy recount from the
delivered x, exactly.  Everything that must not depend on the chunking, the route or the position of the species is compared bit for bit."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile
from tests import dropout_ref as ref

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
    if getattr(eng, "_drop_resident", None) is not sset:
        eng.upload_db(sset.species)
        eng.upload_packed(sset.reads)
        eng.rcls_profile(want_species=False)
        eng.trio_nodes_info()
        bases, _, _, _ = eng.get_node_abundances()
        sset._drop_bases = np.array(bases, copy=True)
        eng._drop_resident = sset
    return sset._drop_bases


def _visits(g):
    v = np.zeros((g.n_nodes, g.n_paths), dtype=bool)
    for h in range(g.n_paths):
        v[g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])], h] = True
    return v


def _selection(species, pick):
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


def _reference(sset, bases, sel_off, sel_hap):
    """tests/dropout_ref.py over every species: computed once per set and left unchanged"""
    node_off = np.concatenate([[0], np.cumsum([g.n_nodes for g in sset.species])])
    out = []
    for s, g in enumerate(sset.species):
        sel = sel_hap[int(sel_off[s]):int(sel_off[s + 1])].astype(np.int64)
        member = _visits(g)[:, sel] if len(sel) else np.zeros((g.n_nodes, 0), dtype=bool)
        out.append(ref.species_dropout(g.node_len, bases[node_off[s]:node_off[s + 1]], member))
    return out


def _check_against_reference(refs, sel_off, got):
    """every entry of `got` against the reference; -> entries solved"""
    from oracle import oracle as orc
    x, obj, status, rows, count = got
    S = len(refs)
    Q = int(sel_off[-1]) + S
    assert len(x) == S and obj.shape == status.shape == (Q,) and rows.shape == (S,) and count.shape == (Q, 4)
    n_solved = 0
    for s, d in enumerate(refs):
        K = int(sel_off[s + 1]) - int(sel_off[s])
        q0 = ref.entry(sel_off, s, 0)
        assert x[s].shape == (K + 1, K)
        assert int(rows[s]) == d["rows"], s
        assert status[q0:q0 + K + 1].tolist() == d["status"].tolist(), (s, status[q0:q0 + K + 1], d["status"])
        if K > 64 or K == 0 or d["rows"] == 0:
            assert not x[s].any() and not obj[q0:q0 + K + 1].any() and not count[q0:q0 + K + 1].any()
            continue
        mask, a = d["mask"], d["a"]
        assert count[q0].tolist() == [d["rows"], 0, 0, 0]
        for e in range(K + 1):
            q = q0 + e
            xg = x[s][e]
            assert np.all(xg >= 0.0) and np.all(xg <= 1.05 * a.max()), (s, e)
            print("species %d entry %d: obj %.17g, objective at x %.17g, oracle %.17g" % (s, e, obj[q], orc.lad_objective(mask, a, xg) * len(a), d["obj"][e]))
            assert orc.lad_objective(mask, a, xg) * len(a) == pytest.approx(obj[q], rel=1e-9, abs=1e-12), (s, e)
            assert obj[q] == pytest.approx(d["obj"][e], rel=1e-9, abs=1e-12), (s, e, obj[q], d["obj"][e])
            if e >= 1:
                k = e - 1
                assert xg[k] == 0.0 and not np.signbit(xg[k]), (s, e)
                assert obj[q] >= obj[q0] * (1 - 1e-9), (s, e)
                assert obj[q] >= a[mask == np.uint64(1 << k)].sum() * (1 - 1e-12), (s, e)
                assert count[q].tolist() == ref.counts(mask, a, x[s][0], xg, k).tolist(), (s, e)
            n_solved += 1
    return n_solved


def _flat(got):
    x, obj, status, rows, count = got
    return [np.concatenate([b.ravel() for b in x]) if len(x) else np.zeros(0), obj, status, rows, count]


def _same(a, b):
    for p, q in zip(_flat(a), _flat(b)):
        assert p.dtype == q.dtype and p.shape == q.shape and p.tobytes() == q.tobytes()


# ---- K_s in {1, 2, 3, 16, 17, 64, 65, 0}, a species without coverage; chunks of one round, two and all; both routes

@pytest.fixture(scope="module")
def mixed():
    import synthdata as synth
    rng = np.random.default_rng(941)
    haps = [1, 2, 3, 16, 17, 64, 65, 4, 5]
    species, start = [], 1
    for s, h in enumerate(haps):
        g = synth.make_species(rng, str(2000 + s), h, 8000 if h < 64 else 4000, start, "GCF_%06d" % (s + 1), present_frac=0.5)
        if s == 8:
            g.truth_depth[:] = 0.0                                           # no read of this species: no covered node
        species.append(g)
        start = g.range_end + 1
    sset = synth.SyntheticSet(species, synth.make_reads(rng, species, 6000))
    shuffle = np.random.default_rng(6)
    # every haplotype of the species in a shuffled order (column = position in the list, not haplotype index); none of species 7
    sset.sel = _selection(species, lambda s, H: [] if s == 7 else [int(h) for h in shuffle.permutation(H)])
    return sset


@pytest.fixture(scope="module")
def mixed_run(eng, mixed):
    bases = _coverage(eng, mixed)
    return bases, eng.strain_dropout(*mixed.sel), _reference(mixed, bases, *mixed.sel)


def test_dropout_every_entry_against_the_oracle(eng, mixed, mixed_run):
    sset = mixed
    bases, got, refs = mixed_run
    K = np.diff(sset.sel[0]).astype(int).tolist()
    assert K == [1, 2, 3, 16, 17, 64, 65, 0, 5]                                # both solver instances and both objective instances, the limit, nothing selected
    assert all(200 <= g.n_nodes <= 2000 for g in sset.species[1:])
    x, obj, status, rows, count = got
    n_solved = _check_against_reference(refs, sset.sel[0], got)
    assert n_solved == sum(k + 1 for k in K[:6])                               # the six covered species with 1 .. 64 columns, every entry
    q6, q7, q8 = (ref.entry(sset.sel[0], s, 0) for s in (6, 7, 8))
    assert np.all(status[q6:q6 + 66] == E_LIMIT) and status[q7] == 1 and np.all(status[q8:q8 + 6] == 1) and rows[8] == 0 and rows[6] == 0
    # K_s = 1: without its one strain the species explains nothing
    d0 = refs[0]
    assert x[0][1][0] == 0.0 and obj[1] == pytest.approx(d0["a"].sum(), rel=1e-12) and count[1][0] == count[1][1] == rows[0] > 0
    print("K = 1: x0 %.17g, rows %d, n_worse %d, n_better %d, rows with a < x0 / 2: %d" % (x[0][0][0], rows[0], count[1][2], count[1][3], int((d0["a"] < x[0][0][0] / 2).sum())))
    assert count[1][3] == 0
    # some strain is needed, and some entry moves rows both ways
    assert any(obj[ref.entry(sset.sel[0], s, e)] > 1.01 * obj[ref.entry(sset.sel[0], s, 0)] for s in range(1, 6) for e in range(1, K[s] + 1))
    assert count[:, 2].max() > 0 and count[:, 3].max() > 0


def test_dropout_chunks_routes_same_bits(eng, mixed, mixed_run, set_opt):
    from pantax_amd._ffi import PantaxHipError
    sset = mixed
    bases, got, refs = mixed_run
    P = sum(len(np.unique(d["mask"])) for d in refs)                           # the base patterns: runs of equal (species, mask)
    for cap in (P + 1, 2 * (P + 1), 3 * (P + 1) - 1):                          # one round a chunk; two; (all of them: the default above)
        set_opt(eng, "dropout_patterns_max", cap)
        _same(eng.strain_dropout(*sset.sel), got)
    set_opt(eng, "dropout_patterns_max", P)                                    # not even one round: refused, and the reason says so
    with pytest.raises(PantaxHipError) as e:
        eng.strain_dropout(*sset.sel)
    assert e.value.code == E_LIMIT and "dropout_patterns_max" in str(e.value)
    set_opt(eng, "dropout_patterns_max", None)
    set_opt(eng, "dropout_route", "walk")
    _same(eng.strain_dropout(*sset.sel), got)
    set_opt(eng, "dropout_route", None)
    # two calls in a row, and a call behind the bootstrap on the same coverage result
    _same(eng.strain_dropout(*sset.sel), got)
    eng.strain_bootstrap(*sset.sel, np.arange(len(sset.species), dtype=np.uint64), n_replicates=1)
    _same(eng.strain_dropout(*sset.sel), got)
    # the refit is the bootstrap's replicate 0 on the same rows
    xb, objb, rowsb, _ = eng.strain_bootstrap(*sset.sel, np.arange(len(sset.species), dtype=np.uint64), n_replicates=0)
    assert np.array_equal(rowsb[0], got[3])
    for s in range(len(sset.species)):
        assert objb[0, s] == pytest.approx(got[1][ref.entry(sset.sel[0], s, 0)], rel=1e-9, abs=1e-12)


# ---- crafted graphs: two haplotypes with the same walk beside a third strain; a strain with covered private nodes; selected haplotypes the refit puts at zero

@pytest.fixture(scope="module")
def crafted():
    import synthdata as synth
    rng = np.random.default_rng(942)
    species, start = [], 1
    # 0: haplotypes 0 and 1 walk nodes 0 .. 23, haplotype 2 walks 12 .. 35
    species.append(_custom("5000", np.full(36, 60), [list(range(24)), list(range(24)), list(range(12, 36))], start, [6.0, 0.0, 3.0]))
    start = species[-1].range_end + 1
    # 1: haplotype 0 walks 0 .. 29 (0 .. 5 private), haplotype 1 walks 10 .. 39 (34 .. 39 private); haplotypes 2 .. 5 have no reads of their own and walk
    # stretches of the others
    walks = [list(range(30)), list(range(10, 40)), list(range(10, 22)), list(range(16, 30)), list(range(6, 16)), list(range(24, 34))]
    species.append(_custom("5001", np.full(40, 60), walks, start, [5.0, 8.0, 0.0, 0.0, 0.0, 0.0]))
    sset = synth.SyntheticSet(species, synth.make_reads(rng, species, 1500, adversarial_frac=0.0))
    sset.sel = _selection(species, lambda s, H: list(range(H)))
    return sset


def test_dropout_crafted_graphs(eng, crafted):
    """Two equal columns: a vertex of the LP holds at most one of them, so one twin sits at zero in the refit.  Dropping the other moves its coverage to
    the first at no cost (its substitute is the twin, gain = what it held); dropping the one at zero changes nothing, and by the helper's rule (a gain
    must be positive) it has no substitute."""
    from pantax_amd.engine import dropout_substitute
    sset = crafted
    bases = _coverage(eng, sset)
    got = eng.strain_dropout(*sset.sel)
    refs = _reference(sset, bases, *sset.sel)
    assert _check_against_reference(refs, sset.sel[0], got) == 4 + 7
    x, obj, status, rows, count = got
    # the twins
    for who, xs, objs in (("device", x[0], obj[0:4]), ("reference", refs[0]["x"], refs[0]["obj"])):
        assert objs[0] > 0 and max(xs[0][0], xs[0][1]) > 3.0, who
        for k, other in ((0, 1), (1, 0)):
            print("%s twin %d: refit %.17g, delta %.3g of %.17g" % (who, k, xs[0][k], objs[k + 1] - objs[0], objs[0]))
            assert objs[k + 1] - objs[0] <= 1e-9 * objs[0], (who, k)
            j, gain, shift = dropout_substitute(k, xs[0], xs[k + 1])
            if xs[0][k] > 0.0:
                assert j == other and gain == pytest.approx(xs[0][k], rel=1e-9), (who, k)
            else:
                assert j == -1 and xs[0][other] > 0.0, (who, k)
    assert count[1][:2].tolist() == count[2][:2].tolist() == [int(rows[0]) - int(count[3][1]), 0] and count[3][1] > 0
    assert obj[3] - obj[0] > 0                                                  # the third strain has covered nodes of its own
    # covered private nodes: needed
    q0 = ref.entry(sset.sel[0], 1, 0)
    for k in (0, 1):
        assert obj[q0 + 1 + k] - obj[q0] > 0 and count[q0 + 1 + k][1] > 0 and refs[1]["obj"][1 + k] - refs[1]["obj"][0] > 0
    # selected haplotypes the refit puts at exactly 0, in the reference and on the device: nothing changes without them
    at_zero = [k for k in range(2, 6) if refs[1]["x"][0][k] == 0.0 and x[1][0][k] == 0.0]
    print("refit of species 1: device %s, reference %s" % (x[1][0].tolist(), refs[1]["x"][0].tolist()))
    assert at_zero
    for k in at_zero:
        assert refs[1]["obj"][1 + k] - refs[1]["obj"][0] <= 1e-9 * refs[1]["obj"][0]
        assert obj[q0 + 1 + k] - obj[q0] <= 1e-9 * obj[q0] and count[q0 + 1 + k][2] == 0, k


# ---- the position of the species in the db

def test_dropout_species_position(eng):
    """the same species at index 0 of one db and at index 2 of another: the same bits"""
    import synthdata as synth
    rng = np.random.default_rng(943)
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
    r1 = eng.strain_dropout([0, 4], sel_x)
    b3 = _coverage(eng, three)
    assert np.array_equal(b3[-X.n_nodes:], b1) and b1.any() and not b3[:-X.n_nodes].any()
    r3 = eng.strain_dropout([0, 2, 2, 6], [1, 0] + sel_x)
    # species 2 of the second db: entries 4 .. 8 of 9 (two columns and three entries, then the one entry of the species without a selection, before it)
    assert r3[0][2].tobytes() == r1[0][0].tobytes() and r3[1][4:].tobytes() == r1[1].tobytes() and r3[4][4:].tobytes() == r1[4].tobytes()
    assert np.array_equal(r3[2][4:], r1[2]) and r3[3][2] == r1[3][0] > 0 and np.all(r1[2] == 0)
    assert np.all(r3[2][:4] == 1) and r1[0][0].std(axis=0).max() > 0


# ---- state and arguments

def _raw(eng, sel_off, sel_hap, n_species=None, fill=77):
    from pantax_amd import _ffi
    so, sh = np.ascontiguousarray(sel_off, dtype=np.uint64), np.ascontiguousarray(sel_hap, dtype=np.uint32)
    cs = _ffi.EvidenceSet(eng.S if n_species is None else n_species, so.ctypes.data, sh.ctypes.data if len(sh) else None)
    Q = len(sh) + eng.S
    K = np.diff(so.astype(np.int64))
    x = np.full(max(int(((K + 1) * K).sum()), 1), float(fill))
    obj = np.full(Q, float(fill))
    st = np.full(Q, fill, dtype=np.int32)
    rows = np.full(eng.S, fill, dtype=np.uint64)
    cnt = np.full((Q, 4), fill, dtype=np.uint64)
    rc = eng.lib.pantax_hip_strain_dropout(eng.ctx, eng.db, C.byref(cs), _ffi.p(x), _ffi.p(obj), _ffi.p(st), _ffi.p(rows), _ffi.p(cnt))
    return rc, (x, obj, st, rows, cnt)


def _untouched(out, fill=77):
    return all(np.all(a == fill) for a in out)


def test_dropout_state_and_arguments(eng, mixed, set_opt):
    from pantax_amd._ffi import PantaxHipError
    sset = mixed
    eng._drop_resident = None
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    sel_off, sel_hap = sset.sel
    rc, out = _raw(eng, sel_off, sel_hap)
    assert rc == E_STATE and _untouched(out)                                   # no coverage pass yet
    eng.get_node_abundances(fetch=False)
    rc, out = _raw(eng, sel_off, sel_hap)
    assert rc == 0 and not _untouched(out)
    good = out
    twice = sel_hap.copy()
    twice[2] = twice[1]                                                        # species 1: a haplotype twice
    beyond = sel_hap.copy()
    beyond[0] = 1                                                              # species 0 has one haplotype
    for args, kw in (((sel_off, twice), {}), ((sel_off, beyond), {}), ((sel_off[:-1], sel_hap[:int(sel_off[-2])]), {"n_species": eng.S - 1})):
        rc, out = _raw(eng, *args, **kw)
        assert rc == E_INVALID and _untouched(out)
    set_opt(eng, "dropout_patterns_max", 1)                                    # a limit of the call's own: the outputs are left as given
    rc, out = _raw(eng, sel_off, sel_hap)
    assert rc == E_LIMIT and _untouched(out)
    set_opt(eng, "dropout_patterns_max", None)
    eng.profile_step(sset.avg_len())                                           # a resident step may zero the arena
    with pytest.raises(PantaxHipError) as e:
        eng.strain_dropout(sel_off, sel_hap)
    assert e.value.code == E_STATE and "resident step" in str(e.value)
    rc, out = _raw(eng, sel_off, sel_hap)
    assert rc == E_STATE and _untouched(out)
    eng.get_node_abundances(fetch=False)
    rc, out = _raw(eng, sel_off, sel_hap)
    assert rc == 0 and all(p.tobytes() == q.tobytes() for p, q in zip(out, good))


# ---- the file seam -----------------------------------------------------------------------------------------------------------

HEADER = ["species_taxid", "strain_taxid", "genome_ID", "class", "predicted_coverage", "refit", "n_rows", "objective", "objective_without", "delta", "delta_fraction",
          "n_member", "n_only", "n_worse", "n_better", "substitute_strain_taxid", "substitute_genome_ID", "substitute_gain", "shift"]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from tests.helpers import seam_world
    yield from seam_world(tmp_path_factory, "pantax_drop", 32, 4, 5, 30000, 30000, present_frac=0.4, single_strain_every=4, with_ids=True)


def _stage_resident(eng, sset):
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    eng.get_node_abundances(fetch=False)


def _picked(sset, db, table):
    """per species: (haplotype, row of the table), ascending haplotype = column order -> (picked, sel_off, sel_hap)"""
    names = [g.name for g in sset.species]
    genome_hap = {r[0]: r[0].split("_ASM")[0] for r in _lines(db / "genomes_info.txt")[1:]}
    picked = [[] for _ in names]
    for i, t in enumerate(table):
        s = names.index(t[0])
        picked[s].append((sset.species[s].hap_names.index(genome_hap[t[2]]), i))
    for p in picked:
        p.sort()
    sel_off = np.concatenate([[0], np.cumsum([len(p) for p in picked])]).astype(np.uint64)
    sel_hap = np.array([h for p in picked for h, _ in p], dtype=np.uint32)
    return picked, sel_off, sel_hap


def test_profile_seam_strain_dropout(world, set_opt, monkeypatch):
    from pantax_amd import _ffi
    from pantax_amd._ffi import PantaxHipError
    from pantax_amd.engine import dropout_substitute
    sset, root, db, gaf, eng = world
    _profile(eng, db, root / "wd_plain", gaf)
    wd = root / "wd_drop"
    set_opt(eng, "db_groups", 1)
    _profile(eng, db, wd, gaf, strain_dropout_file=str(wd / "drop.tsv"))
    for f in ("species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt"):   # the option changes none of the tables
        assert open(wd / f, "rb").read() == open(root / "wd_plain" / f, "rb").read()
    assert not os.path.exists(root / "wd_plain" / "drop.tsv")
    rows = _lines(wd / "drop.tsv")
    assert rows[0] == HEADER and all(len(r) == len(HEADER) for r in rows)
    rows = rows[1:]
    table = _lines(wd / "strain_abundance.txt")[1:]
    n_str = len(table)
    assert n_str >= 2 and [tuple(r[:4]) for r in rows[:n_str]] == [tuple(t[:3]) + ("strain",) for t in table]
    assert all(np.float64(rows[i][4]) == np.float64(table[i][3]) for i in range(n_str))
    sp_rows = rows[n_str:]
    assert all(r[1] == "-" and r[2] == "-" and r[3] == "species" for r in sp_rows)
    # the stage call of the same sample for the table's rows: every cell recomputes from its outputs
    _stage_resident(eng, sset)
    names = [g.name for g in sset.species]
    picked, sel_off, sel_hap = _picked(sset, db, table)
    x, obj, status, nrows, count = eng.strain_dropout(sel_off, sel_hap)
    place = {i: (s, k) for s, p in enumerate(picked) for k, (_, i) in enumerate(p)}
    n_needed = n_sub = 0
    for i in range(n_str):
        s, k = place[i]
        q0 = ref.entry(sel_off, s, 0)
        r = rows[i]
        assert status[q0] == 0 and status[q0 + 1 + k] == 0
        assert np.float64(r[5]) == x[s][0][k] and int(r[6]) == int(nrows[s]) and np.float64(r[7]) == obj[q0] and np.float64(r[8]) == obj[q0 + 1 + k]
        delta = obj[q0 + 1 + k] - obj[q0]
        assert np.float64(r[9]) == delta and (r[10] == "-" if obj[q0 + 1 + k] == 0 else np.float64(r[10]) == delta / obj[q0 + 1 + k])
        assert [int(c) for c in r[11:15]] == count[q0 + 1 + k].tolist()
        j, gain, shift = dropout_substitute(k, x[s][0], x[s][k + 1])
        if j < 0:
            assert r[15:18] == ["-", "-", "-"]
        else:
            sub = table[picked[s][j][1]]
            assert r[15:17] == sub[1:3] and np.float64(r[17]) == gain
            n_sub += 1
        assert np.float64(r[18]) == shift
        n_needed += int(delta > 0)
    assert n_needed >= 1 and n_sub >= 1
    seq = [r[0] for r in sp_rows]
    sp_table = [r[0] for r in _lines(wd / "species_abundance.txt")[1:]]      # the run takes the selected species in the order of the species table
    assert len(set(seq)) == len(seq) >= 2 and seq == [t for t in sp_table if t in set(seq)] and {t[0] for t in table} == set(seq)
    for r in sp_rows:
        s = names.index(r[0])
        assert int(r[6]) == int(nrows[s]) and np.float64(r[7]) == obj[ref.entry(sel_off, s, 0)] and r[4:6] == ["-", "-"] and r[8:] == ["-"] * 11
    # the same file from a run cut into three groups of species, and from one cut by the path steps a resident db may hold
    wg = root / "wd_drop_groups"
    set_opt(eng, "db_groups", 3)
    _profile(eng, db, wg, gaf, strain_dropout_file=str(wg / "drop.tsv"))
    set_opt(eng, "db_groups", None)
    assert open(wg / "drop.tsv", "rb").read() == open(wd / "drop.tsv", "rb").read()
    ws = root / "wd_drop_steps"
    set_opt(eng, "db_path_steps_max", int(max(len(g.path_nodes) for g in sset.species) * 3))
    _profile(eng, db, ws, gaf, strain_dropout_file=str(ws / "drop.tsv"))
    set_opt(eng, "db_path_steps_max", None)
    assert open(ws / "drop.tsv", "rb").read() == open(wd / "drop.tsv", "rb").read()
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_drop_cli"
    wc.mkdir()
    run = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0",
                          "--strain-dropout", str(wc / "drop.tsv")], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert open(wc / "drop.tsv", "rb").read() == open(wd / "drop.tsv", "rb").read()
    # beside the bootstrap and the model fit: the same bytes
    wb = root / "wd_drop_all"
    _profile(eng, db, wb, gaf, strain_fit_file=str(wb / "fit.tsv"), strain_bootstrap_file=str(wb / "boot.tsv"), strain_bootstrap_replicates=2, strain_dropout_file=str(wb / "drop.tsv"))
    assert open(wb / "drop.tsv", "rb").read() == open(wd / "drop.tsv", "rb").read() and os.path.exists(wb / "boot.tsv") and os.path.exists(wb / "fit.tsv")
    # several ranks: refused with the plan's wording
    for rank in range(2):
        wn = root / ("wd_drop_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, strain_dropout_file=str(wn / "drop.tsv"))
        assert e.value.code == E_INVALID and "the leave-one-out report (strain_dropout_file) needs one rank and an unsharded ingest (world_size 2)" in str(e.value)
        assert not os.path.exists(wn / "drop.tsv") and not os.path.exists(wn / "species_abundance.txt")
    # a caller compiled against the header before this field: its struct ends behind strain_bootstrap_seed, the report reads as off
    real = _ffi.ProfileExt

    class OldExt(real):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.struct_size = 40

    monkeypatch.setattr(_ffi, "ProfileExt", OldExt)
    wo = root / "wd_drop_old"
    _profile(eng, db, wo, gaf, strain_bootstrap_file=str(wo / "boot.tsv"), strain_bootstrap_replicates=2, strain_dropout_file=str(wo / "drop.tsv"))
    monkeypatch.setattr(_ffi, "ProfileExt", real)
    assert os.path.exists(wo / "boot.tsv") and not os.path.exists(wo / "drop.tsv")
    assert open(wo / "strain_abundance.txt", "rb").read() == open(wd / "strain_abundance.txt", "rb").read()


def test_profile_seam_dropout_skips_a_species_of_65_rows(tmp_path_factory):
    """a species with more rows in strain_abundance.txt than the call serves prints `skipped`, its strains dashes; the species beside it is served"""
    import synthdata as synth
    from pantax_amd.engine import Engine
    rng = np.random.default_rng(944)
    wide = synth.make_species(rng, "7000", 100, 30000, 1, "GCF_W", present_frac=1.0)
    small = synth.make_species(rng, "7001", 3, 8000, wide.range_end + 1, "GCF_S", present_frac=1.0)
    sset = synth.SyntheticSet([wide, small], synth.make_reads(rng, [wide, small], 60000, adversarial_frac=0.0, with_ids=True))
    root = tmp_path_factory.mktemp("pantax_drop_wide")
    db = root / "db"
    db.mkdir()
    synth.write_db(sset, str(db))
    gaf = root / "gfa_mapped.gaf"
    synth.write_gaf(sset.reads, str(gaf))
    eng = Engine(0)
    try:
        wd = root / "wd"
        _profile(eng, db, wd, gaf, fr=0.0, fc=1e9, sd=1e9, strain_dropout_file=str(wd / "drop.tsv"))
    finally:
        eng.close()
    table = _lines(wd / "strain_abundance.txt")[1:]
    n_wide = sum(1 for t in table if t[0] == "7000")
    print("rows of the wide species in the strain table: %d" % n_wide)
    assert n_wide >= 65
    rows = _lines(wd / "drop.tsv")[1:]
    strains, sp_rows = rows[:len(table)], rows[len(table):]
    assert all(r[5:] == ["-"] * 14 for r in strains if r[0] == "7000") and any(r[5] != "-" for r in strains if r[0] == "7001")
    by = {r[0]: r for r in sp_rows}
    assert by["7000"][3] == "skipped" and by["7000"][6] == "0" and by["7000"][7] == "-" and by["7001"][3] == "species" and by["7001"][7] != "-"
