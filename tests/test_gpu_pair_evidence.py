"""GPU tests of the pairwise strain evidence (pantax_hip_strain_pair_evidence, --strain-pair-evidence).  The expected values come from the numpy
restatement of the contract in tests/pair_evidence_ref.py (pinned by tests/test_pair_evidence_ref.py on a hand-computed case), applied to the
bases_per_node and node_base_cov that get_node_abundances hands out.  Everything is an integer: every comparison is np.array_equal.  Each stage case runs
under the default membership route and under hap_pairs_route=walk, and under the default chunk of the node pass and under a small one (option
hap_pairs_chunk), and is tied to pantax_hip_db_hap_pairs and pantax_hip_strain_evidence on the same selection."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile, seam_world
from tests.pair_evidence_ref import HEADER, pair_evidence, table
from tests.test_gpu_evidence import _coverage, _mixed_set, _selection

pytestmark = pytest.mark.gpu

CHUNK_MIN = 1024       # the node pass cuts a species' nodes into chunks of max(1024, 32 ka kb) nodes per block pair (hap_pairs_plan.hpp), taken 64 at a time
E_INVALID, E_LIMIT, E_STATE = -1, -4, -7


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _check(got, exp):
    assert len(got) == len(exp) == 3
    for a, b in zip(got, exp):
        assert a.dtype == b.dtype == np.uint64 and a.shape == b.shape and np.array_equal(a, b)


def _all_ways(eng, set_opt, sel, small_chunk=128):
    """the call under the default route and under hap_pairs_route=walk, each with the default chunk and with a small one: the same numbers four times"""
    got = eng.pair_evidence(*sel)
    for route, chunk in ((None, small_chunk), ("walk", None), ("walk", small_chunk)):
        set_opt(eng, "hap_pairs_route", route)
        set_opt(eng, "hap_pairs_chunk", chunk)
        try:
            _check(eng.pair_evidence(*sel), got)
        finally:
            set_opt(eng, "hap_pairs_route", None)
            set_opt(eng, "hap_pairs_chunk", None)
    return got


def _block(res, s):
    """the K x K x 4 block of species s of a (pair_off, pair, species) result"""
    lo, hi = int(res[0][s]), int(res[0][s + 1])
    K = int(round((hi - lo) ** 0.5))
    assert K * K == hi - lo
    return res[1][lo:hi].reshape(K, K, 4)


def _identities(eng, sel, res):
    """the identities of the header: against the db-only call and the evidence call on the same selection, and within the result"""
    hp = eng.hap_pairs(*sel)
    hap, sp = eng.strain_evidence(*sel)
    assert np.array_equal(res[0], hp[0]) and np.array_equal(res[1][:, :2], hp[1])            # columns 0:2 = pantax_hip_db_hap_pairs
    assert np.array_equal(res[2], sp) and np.array_equal(res[2][:, :, :2], hp[2])            # species sums = the evidence call's
    diag = [np.einsum("iiq->iq", _block(res, s)) for s in range(len(res[2]))]
    assert np.array_equal(np.concatenate(diag) if diag else np.zeros((0, 4), dtype=np.uint64), hap[:, 0])   # the diagonal = the evidence call's all
    for s in range(len(res[2])):
        P, d = _block(res, s), diag[s]
        assert np.array_equal(P, P.transpose(1, 0, 2))
        assert np.all(P <= np.minimum(d[:, None], d[None, :])) and (len(P) == 0 or np.all(res[2][s, 2] <= P))


@pytest.fixture(scope="module")
def narrow():
    import synthdata as synth
    return synth.make_set(921, 3, 6, 20000, 30000, present_frac=0.6)


def test_pair_evidence_narrow_routes_and_selections(eng, narrow, set_opt):
    """all haplotypes of one species, a shuffled three of the next, none of the last; by the node -> haplotype words and by the walks"""
    species = narrow.species
    bases, cov = _coverage(eng, narrow)
    sel = _selection(species, lambda s, H: range(H) if s == 0 else ([] if s == 2 else [4, 0, 2]))
    exp = pair_evidence(species, *sel, cov, bases)
    # the case holds what the kernel can get wrong (computed from the set: a changed generator cannot hollow the test out)
    V = [g.n_nodes for g in species]
    assert all(g.n_paths == 6 for g in species)                              # <= 64 haplotypes: the default route is the node -> haplotype words
    assert V[0] > max(CHUNK_MIN, 32 * 6 * 6) and V[1] > max(CHUNK_MIN, 32 * 3 * 3)   # a chunk border inside both species under the default chunk
    assert all(v % 64 and (v % CHUNK_MIN) % 64 and (v % 128) % 64 for v in V[:2])    # a last tile that ends inside a wave
    assert exp[0].tolist() == [0, 36, 45, 45]
    for s in (0, 1):
        P = _block(exp, s)
        K = len(P)
        d = np.einsum("iiq->iq", P)
        off = P[~np.eye(K, dtype=bool)]
        lo = np.minimum(d[:, None], d[None, :])[~np.eye(K, dtype=bool)]
        assert np.all(off[:, 2:] > 0) and np.all(off[:, 2:] < lo[:, 2:])     # off-diagonal covered and bases: there, and strictly below the diagonal
        assert np.all(off[:, :2] < lo[:, :2])
    assert np.all(exp[2][:2, 2, 3] > 0) and exp[2][1, 1, 0] > 0              # covered core nodes; nodes none of the three walks
    assert np.array_equal(exp[2][2, 1], exp[2][2, 0]) and not exp[2][2, 2].any()     # nothing selected: every node is an orphan, no core
    got = _all_ways(eng, set_opt, sel)
    _check(got, exp)
    _identities(eng, sel, got)
    again = eng.pair_evidence(*sel, species=False)
    assert again[2] is None and np.array_equal(again[1], exp[1])
    # one haplotype a species: pair = core = the evidence call's all
    one = _selection(species, lambda s, H: [s + 1])
    got1 = _all_ways(eng, set_opt, one)
    _check(got1, pair_evidence(species, *one, cov, bases))
    _identities(eng, one, got1)
    assert all(np.array_equal(_block(got1, s)[0, 0], got1[2][s, 2]) for s in range(3))


def test_pair_evidence_64_and_65_haplotypes(eng, set_opt):
    """bit 63 of the one-word route (haplotype 63 of 64), and the first species with two words (65 haplotypes), where block pair (0, 1) has one live column"""
    sset = _mixed_set(922, [64, 65], 8000, 8000)
    species = sset.species
    assert [g.n_paths for g in species] == [64, 65] and all(g.n_nodes > 128 and g.n_nodes % 64 for g in species)
    bases, cov = _coverage(eng, sset)
    full = _selection(species, lambda s, H: range(H))
    exp = pair_evidence(species, *full, cov, bases)
    assert exp[0].tolist() == [0, 64 * 64, 64 * 64 + 65 * 65]
    P0, P1 = _block(exp, 0), _block(exp, 1)
    assert P0[63, 63, 3] > 0 and np.all(P0[63, :63, 3] > 0)                  # the last bit of the word, against every other, with bases on what they share
    assert P1[64, 64, 3] > 0 and np.all(P1[:64, 64, 3] > 0) and np.any(P1[:64, 64] != P1[64, 64])   # the one column of word 1, against every row of word 0
    got = _all_ways(eng, set_opt, full, small_chunk=64)
    _check(got, exp)
    _identities(eng, full, got)
    part = _selection(species, lambda s, H: [63, 5, 20] if s == 0 else [64, 0, 33])   # a few bits of the word; the wide species through compact masks
    got = _all_ways(eng, set_opt, part)
    _check(got, pair_evidence(species, *part, cov, bases))
    _identities(eng, part, got)


def test_pair_evidence_wide_species(eng, set_opt):
    """130 haplotypes, all selected in shuffled order: three words, six block pairs, the off-diagonal ones mirrored into the lower triangle, four columns each"""
    sset = _mixed_set(923, [130], 8000, 8000)
    species = sset.species
    assert species[0].n_paths == 130
    bases, cov = _coverage(eng, sset)
    order = [int(h) for h in np.random.default_rng(7).permutation(130)]
    sel = _selection(species, lambda s, H: order)
    exp = pair_evidence(species, *sel, cov, bases)
    P = _block(exp, 0)
    d = np.einsum("iiq->iq", P)
    for a, b in ((3, 100), (70, 129), (0, 128), (129, 5), (100, 63)):        # members in different words, both ways round, all four columns their own
        assert a // 64 != b // 64 and np.all(P[a, b] > 0) and np.all(P[a, b] != d[a]) and np.all(P[a, b] != d[b])
        assert P[a, b, 0] < P[a, b, 1] and P[a, b, 2] <= P[a, b, 1] and P[a, b, 3] != P[a, b, 2]
    got = _all_ways(eng, set_opt, sel, small_chunk=64)
    _check(got, exp)
    _identities(eng, sel, got)
    part = _selection(species, lambda s, H: order[:70])                      # two words, six live columns in the second
    _check(_all_ways(eng, set_opt, part), pair_evidence(species, *part, cov, bases))


def _raw(eng, sel_off, sel_hap, cap, n_species=None, fill=77):
    """the C call as it is: (rc, pair_off, pair, species); the arrays are pre-filled with `fill`"""
    from pantax_amd import _ffi
    so, sh = np.ascontiguousarray(sel_off, dtype=np.uint64), np.ascontiguousarray(sel_hap, dtype=np.uint32)
    cs = _ffi.EvidenceSet(eng.S if n_species is None else n_species, so.ctypes.data, sh.ctypes.data if len(sh) else None)
    pair_off = np.full(eng.S + 1, fill, dtype=np.uint64)
    pair = np.full((max(cap, 1), 4), fill, dtype=np.uint64)
    sp = np.full((eng.S, 3, 4), fill, dtype=np.uint64)
    rc = eng.lib.pantax_hip_strain_pair_evidence(eng.ctx, eng.db, C.byref(cs), _ffi.p(pair_off), cap, _ffi.p(pair), _ffi.p(sp))
    return rc, pair_off, pair, sp


def test_pair_evidence_256_served_257_refused(eng, set_opt):
    from pantax_amd._ffi import PantaxHipError
    sset = _mixed_set(925, [257, 3], 3000, 3000)
    species = sset.species
    assert species[0].n_paths == 257
    bases, cov = _coverage(eng, sset)
    wide = _selection(species, lambda s, H: range(H))
    rc, pair_off, pair, sp = _raw(eng, *wide, 257 * 257 + 9)
    assert rc == E_LIMIT and pair_off.tolist() == [0, 257 * 257, 257 * 257 + 9] and np.all(pair == 77) and np.all(sp == 77)
    with pytest.raises(PantaxHipError) as e:
        eng.pair_evidence(*wide)
    assert e.value.code == E_LIMIT and "species 0" in str(e.value) and "257" in str(e.value)
    most = _selection(species, lambda s, H: range(1, H) if s == 0 else [2])  # 256 of them: four full words, ten block pairs
    exp = pair_evidence(species, *most, cov, bases)
    assert exp[0].tolist() == [0, 65536, 65537] and exp[1][:, 3].any()
    got = eng.pair_evidence(*most)
    _check(got, exp)
    _identities(eng, most, got)
    set_opt(eng, "hap_pairs_chunk", 64)
    _check(eng.pair_evidence(*most), exp)


def test_pair_evidence_sizing_state_and_arguments(eng, narrow):
    from pantax_amd._ffi import PantaxHipError
    sset = narrow
    species = sset.species
    eng._ev_resident = None
    eng.upload_db(species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    sel = _selection(species, lambda s, H: [4, 1] if s == 1 else ([H - 1] if s == 0 else []))
    for cap in (0, 5):                                                       # no coverage pass yet: refused whatever the array holds, nothing but pair_off written
        rc, pair_off, pair, sp = _raw(eng, *sel, cap)
        assert rc == E_STATE and pair_off.tolist() == [0, 1, 5, 5] and np.all(pair == 77) and np.all(sp == 77)
    with pytest.raises(PantaxHipError) as e:
        eng.pair_evidence(*sel)
    assert e.value.code == E_STATE and "pantax_hip_node_coverage" in str(e.value)
    bases, cov, _, _ = eng.get_node_abundances()
    exp = pair_evidence(species, *sel, cov, bases)
    # pair_cap = 0 sizes the output; one entry short is still short
    for cap in (0, 4):
        rc, pair_off, pair, sp = _raw(eng, *sel, cap)
        assert rc == E_LIMIT and pair_off.tolist() == [0, 1, 5, 5] and np.all(pair == 77) and np.all(sp == 77)
    rc, pair_off, pair, sp = _raw(eng, *sel, 5)
    assert rc == 0
    _check((pair_off, pair, sp), exp)
    assert exp[1][:, 2].all() and exp[1][:, 3].all()
    # refused arguments: nothing is written
    for args, kw in ((([0, 0, 2, 2], [3, 3]), {}),                           # a haplotype twice within a species
                     (([0, 1, 1, 1], [species[0].n_paths]), {}),             # index = n_paths
                     ((sel[0][:-1], sel[1]), {"n_species": eng.S - 1})):
        rc, pair_off, pair, sp = _raw(eng, *args, 64, **kw)
        assert rc == E_INVALID and np.all(pair == 77) and np.all(sp == 77)
    # nothing selected: no entry, every node of every species is an orphan
    rc, pair_off, pair, sp = _raw(eng, [0, 0, 0, 0], [], 0)
    assert rc == 0 and not pair_off.any() and np.all(pair == 77) and np.array_equal(sp[:, 0], sp[:, 1]) and not sp[:, 2].any()
    assert sp[:, 0, 0].tolist() == [g.n_nodes for g in species] and np.array_equal(sp[:, 0], exp[2][:, 0]) and int(sp[:, 0, 3].sum()) == int(bases.sum())
    # a resident step keeps no node_base_cov and may zero the arena: refused behind it, fine again behind the next stage call
    eng.profile_step(sset.avg_len())
    rc, pair_off, pair, sp = _raw(eng, *sel, 5)
    assert rc == E_STATE and pair_off.tolist() == [0, 1, 5, 5] and np.all(pair == 77) and np.all(sp == 77)
    with pytest.raises(PantaxHipError) as e:
        eng.pair_evidence(*sel)
    assert e.value.code == E_STATE and "resident step" in str(e.value)
    eng.get_node_abundances(fetch=False)
    _check(eng.pair_evidence(*sel), exp)


# ---- the file seam -----------------------------------------------------------------------------------------------------------

SIX = {"read_strain_file": "rs.tsv", "strain_coverage_file": "ct.tsv", "strain_evidence_file": "ev.tsv", "strain_read_support_file": "sup.tsv",
       "strain_depth_file": "dp.tsv", "strain_near_miss_file": "nm.tsv"}
TABLES = ["species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt"]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    yield from seam_world(tmp_path_factory, "pantax_pe", 32, 4, 5, 30000, 30000, present_frac=0.4, single_strain_every=4, with_ids=True)   # the small world of test_gpu_seam_reports.py


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_profile_seam_strain_pair_evidence(world, set_opt, capfd):
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng = world
    # min_cov as test_profile_seam_all_reports_at_once chooses it
    _profile(eng, db, root / "wd_all", gaf)
    covs = sorted(float(r[3]) for r in _lines(root / "wd_all" / "strain_abundance.txt")[1:])
    cuts = [int(c) + 1 for c in covs if sum(x < int(c) + 1 for x in covs) >= 1 and sum(x >= int(c) + 1 for x in covs) >= 2]
    assert cuts, covs
    mc = cuts[0]
    # (a) the pair report beside all six others; (b) the six without it: the tables and the six files do not notice it
    wa, w6 = root / "wd_a", root / "wd_6"
    _profile(eng, db, wa, gaf, min_cov=mc, strain_pair_evidence_file=str(wa / "pe.tsv"), **{k: str(wa / v) for k, v in SIX.items()})
    _profile(eng, db, w6, gaf, min_cov=mc, **{k: str(w6 / v) for k, v in SIX.items()})
    assert not os.path.exists(w6 / "pe.tsv")
    for f in TABLES + list(SIX.values()):
        assert _bytes(w6 / f) == _bytes(wa / f), f
    rows = _lines(wa / "pe.tsv")
    assert rows[0] == HEADER and all(len(r) == len(HEADER) for r in rows)
    tab = _lines(wa / "strain_abundance.txt")[1:]
    names = [g.name for g in sset.species]
    per_species = {n: sum(1 for t in tab if t[0] == n) for n in names}
    assert sum(1 for k in per_species.values() if k >= 2) >= 2               # several species with at least two rows
    assert len(rows) - 1 == 3 * sum(k * (k - 1) // 2 for k in per_species.values())
    # the stage call of the same sample for the table's rows
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    eng.get_node_abundances(fetch=False)
    genome_hap = {r[0]: r[0].split("_ASM")[0] for r in _lines(db / "genomes_info.txt")[1:]}
    picked = [[] for _ in names]                                             # per species: (haplotype, first row of the table), ascending haplotype
    for i, t in enumerate(tab):
        s = names.index(t[0])
        h = sset.species[s].hap_names.index(genome_hap[t[2]])
        if h not in [x for x, _ in picked[s]]:
            picked[s].append((h, i))
    for p in picked:
        p.sort()
    sel_off = np.concatenate([[0], np.cumsum([len(p) for p in picked])]).astype(np.uint64)
    sel_hap = np.array([h for p in picked for h, _ in p], dtype=np.uint32)
    res = eng.pair_evidence(sel_off, sel_hap)
    hap, _ = eng.strain_evidence(sel_off, sel_hap)
    order = [x[0] for x in _lines(wa / "species_abundance.txt")[1:]]         # the run takes the selected species in the order of the species table
    exp = table([(n, [(tab[i][1], tab[i][2], np.float64(tab[i][3])) for _, i in picked[names.index(n)]], _block(res, names.index(n))) for n in order if n in names])
    assert len(exp) == len(rows)
    for r, x in zip(rows[1:], exp[1:]):
        assert r[:10] == x[:10] and r[13] == x[13]
        for c in (10, 11, 12):
            assert r[c] == "-" if isinstance(x[c], str) else np.float64(r[c]) == x[c]
    assert {r[5] for r in rows[1:]} == {"shared", "only"} and any(r[5] == "only" and int(r[9]) > 0 for r in rows[1:]) and any(r[5] == "shared" and int(r[8]) > 0 for r in rows[1:])
    # for every row of a pair, only + shared = the `all` row of the same strain in ev.tsv
    ev_all = {tuple(r[:3]): [int(x) for x in r[4:8]] for r in _lines(wa / "ev.tsv")[1:] if r[3] == "all"}
    ints = lambda r: [int(x) for x in r[6:10]]
    for i in range(1, len(rows), 3):
        sh, oa, ob = rows[i:i + 3]
        assert (sh[5], oa[5], ob[5]) == ("shared", "only", "only") and tuple(oa[:3]) == tuple(sh[:3]) and ob[1:3] == sh[3:5] and ob[3:5] == sh[1:3]
        assert [a + b for a, b in zip(ints(sh), ints(oa))] == ev_all[tuple(oa[:3])]
        assert [a + b for a, b in zip(ints(sh), ints(ob))] == ev_all[tuple(ob[:3])]
        assert len({sh[13], oa[13], ob[13]}) == 1 and sh[13] in ("identical", "nested", "distinct")
    assert all(np.array_equal(np.einsum("iiq->iq", _block(res, s)), hap[int(sel_off[s]):int(sel_off[s + 1]), 0]) for s in range(len(names)))
    # alone, and alone with one species a group: the same bytes, and no other report's file
    wc, wb = root / "wd_c", root / "wd_b"
    _profile(eng, db, wc, gaf, min_cov=mc, strain_pair_evidence_file=str(wc / "pe.tsv"))
    set_opt(eng, "db_path_steps_max", 1)
    try:
        _profile(eng, db, wb, gaf, min_cov=mc, strain_pair_evidence_file=str(wb / "pe.tsv"))
    finally:
        set_opt(eng, "db_path_steps_max", None)
    for w in (wc, wb):
        assert _bytes(w / "pe.tsv") == _bytes(wa / "pe.tsv")
        assert not any((w / o).exists() for o in SIX.values())
        for f in TABLES:
            assert _bytes(w / f) == _bytes(wa / f), f
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wl = root / "wd_cli"
    wl.mkdir()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wl), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0", "--min_cov", str(mc),
                        "--strain-pair-evidence", str(wl / "pe.tsv")], cwd=str(wl), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert _bytes(wl / "pe.tsv") == _bytes(wa / "pe.tsv")
    # a call that runs no strain step writes no file and says so; "None" and "" are off
    wr = root / "wd_species_only"
    capfd.readouterr()
    _profile(eng, db, wr, gaf, species=True, strain=False, min_cov=mc, strain_pair_evidence_file=str(wr / "pe_species.tsv"))
    assert not os.path.exists(wr / "pe_species.tsv") and "no strain step" in capfd.readouterr().err
    for off in ("None", ""):
        wo = root / ("wd_off_%d" % len(off))
        _profile(eng, db, wo, gaf, min_cov=mc, strain_pair_evidence_file=off)
        assert not os.path.exists(wo / "None") and sorted(os.listdir(wo)) == sorted(os.listdir(root / "wd_all"))
    # several ranks
    wn = root / "wd_ranks"
    with pytest.raises(PantaxHipError) as e:
        _profile(eng, db, wn, gaf, rank=0, world_size=2, allreduce=lambda buf: None, strain_pair_evidence_file=str(wn / "pe.tsv"))
    assert e.value.code == E_INVALID and "strain_pair_evidence_file" in str(e.value)
    assert not os.path.exists(wn / "pe.tsv") and not os.path.exists(wn / "species_abundance.txt")
