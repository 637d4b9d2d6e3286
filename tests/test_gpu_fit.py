"""GPU tests of the model fit per strain (pantax_hip_strain_fit, --strain-fit).  The expected values come from the numpy restatement of the contract in
tests/fit_ref.py (pinned by tests/test_fit_ref.py on a hand-computed case), applied to the bases_per_node that get_node_abundances hands out -- the
parity tests pin those against the oracle.  E(v) is a deterministic function of the inputs and every sum an integer: every comparison is np.array_equal.
The sets are the recipes of tests/test_gpu_evidence.py, whose shapes hit the borders of the node pass; each case asserts its borders from the set."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile, seam_world
from tests.fit_ref import check_identities, fit

pytestmark = pytest.mark.gpu

CHUNK = 1024       # the node pass cuts every species' nodes into chunks of 1024 (a wave each), taken in tiles of 256, 64 lanes wide
E_INVALID, E_STATE = -1, -7
TINY = 2.0 ** -54


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _coverage(eng, sset):
    """the set resident with a coverage result of the stage kind -> bases_per_node; computed once per set"""
    if getattr(eng, "_fit_resident", None) is not sset:
        eng.upload_db(sset.species)
        eng.upload_packed(sset.reads)
        eng.rcls_profile(want_species=False)
        eng.trio_nodes_info()
        bases, _, _, _ = eng.get_node_abundances()
        sset._fit_bases = np.array(bases, copy=True)
        eng._fit_resident = sset
    return sset._fit_bases


def _selection(species, pick):
    """pick(s, H) -> [(haplotype, weight)] of species s -> (sel_off, sel_hap, sel_w)"""
    off, hp, w = [0], [], []
    for s, g in enumerate(species):
        for h, x in pick(s, g.n_paths):
            hp.append(h)
            w.append(x)
        off.append(len(hp))
    return np.array(off, dtype=np.uint64), np.array(hp, dtype=np.uint32), np.array(w, dtype=np.float64)


def _visits(g):
    """node-level membership of a graph: bool [V, H]"""
    v = np.zeros((g.n_nodes, g.n_paths), dtype=bool)
    for h in range(g.n_paths):
        v[g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])], h] = True
    return v


def _check(got, exp):
    for a, b in zip(got, exp):
        assert a.dtype == b.dtype == np.uint64 and a.shape == b.shape and np.array_equal(a, b)


def _both_routes(eng, set_opt, sel):
    """the call under the default route and under fit_route=walk: the same numbers"""
    got = eng.strain_fit(*sel)
    set_opt(eng, "fit_route", "walk")
    try:
        walk = eng.strain_fit(*sel)
    finally:
        set_opt(eng, "fit_route", None)
    _check(walk, got)
    return got


@pytest.fixture(scope="module")
def narrow():
    import synthdata as synth
    return synth.make_set(921, 3, 6, 20000, 30000, present_frac=0.6)


def narrow_case(sset):
    """all of species 0 with weights that tie, a zero and a small one; [4, 0, 2] of species 1 with a sum that depends on its order; none of species 2.
    The borders are asserted from the set: a changed generator cannot hollow the test out"""
    w0 = [0.5, 1.5, 2.25, 0.0, 1e-3, 40.5]
    w1 = {4: 0.5, 0: TINY, 2: TINY}                                          # the list order differs from the index order
    sel = _selection(sset.species, lambda s, H: list(zip(range(H), w0)) if s == 0 else ([] if s == 2 else [(h, w1[h]) for h in (4, 0, 2)]))
    V = [g.n_nodes for g in sset.species]
    assert all(g.n_paths == 6 for g in sset.species)                         # <= 64 haplotypes: the default route is the node -> haplotype words
    assert any(v % 64 and v % CHUNK for v in V)                              # a last tile that ends inside a wave
    assert any(v > CHUNK for v in V)                                         # a chunk border inside a species
    g = sset.species[1]
    vis = _visits(g)
    # walked by 0, 2 and 4: in index order p = (2^-54 + 2^-54) + 0.5 = 0.5 + 2^-53, and a length of 4k + 1 puts t just above the tie 2k + 0.5: E = 2k + 1.
    # Added in list order p = 0.5 and t IS the tie: E = 2k -- an implementation that adds in list order fails on these nodes
    odd = vis[:, 0] & vis[:, 2] & vis[:, 4] & (np.asarray(g.node_len) % 4 == 1)
    assert odd.sum() > 0
    g0 = sset.species[0]
    vis0 = _visits(g0)
    only0 = vis0[:, 0] & (vis0.sum(axis=1) == 1)                             # p = 0.5 alone: ties wherever the length is odd
    assert (np.asarray(g0.node_len)[only0] % 2 == 1).any()
    return sel


def test_fit_narrow_order_ties_and_routes(eng, narrow, set_opt):
    sset = narrow
    bases = _coverage(eng, sset)
    sel = narrow_case(sset)
    exp = fit(sset.species, *sel, bases)
    hap, sp = exp
    assert hap[:, 0, 4].all() and hap[:6, 0, 5].all() and hap[:, :, 6].sum() > 0 and sp[0, 0, 6] > 0   # excess, deficit and blind nodes
    assert hap[3, 1, 3] == 0 and hap[3, 1, 2] > 0 and hap[3, 0, 3] > 0       # the zero weight alone predicts nothing on its private nodes
    assert sp[1, 2, 0] > 0 and np.array_equal(sp[2, 0], sp[2, 2]) and not sp[2, 1].any()   # orphans beside a selection; a species without one is all orphan
    check_identities(*exp)
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


def test_fit_64_and_65_haplotypes(eng, set_opt):
    """the last bit of the one-word route (haplotype 63 of 64), the first species beyond it (65 haplotypes: compact masks), and every haplotype selected:
    K = 65 is two words with one entry in the second"""
    sset = _mixed_set(922, [64, 65], 8000, 8000)
    assert [g.n_paths for g in sset.species] == [64, 65]
    bases = _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: [(63, 0.7), (5, 1.3), (20, 0.45)] if s == 0 else [(64, 0.9), (0, 0.35), (33, 1.1)])
    exp = fit(sset.species, *sel, bases)
    assert exp[0][0, 0, 3] > 0 and exp[0][3, 0, 3] > 0 and np.all(exp[1][:, 2, 0] > 0)
    _check(_both_routes(eng, set_opt, sel), exp)
    full = _selection(sset.species, lambda s, H: [(h, 0.0137 * (h + 1)) for h in range(H)])
    exp = fit(sset.species, *full, bases)
    assert exp[0][64 + 64, 0, 3] > 0                                         # the entry of the second word predicts bases
    check_identities(*exp)
    _check(_both_routes(eng, set_opt, full), exp)


def wide_case(sset):
    """80 of 100 haplotypes in shuffled order with distinct weights: two mask words per node, p(v) summed across both in index order"""
    rng = np.random.default_rng(7)
    pick0 = [int(h) for h in rng.permutation(100)[:80]]
    w = {h: 0.05 + 0.013 * i for i, h in enumerate(pick0)}
    sel = _selection(sset.species, lambda s, H: [(h, w[h]) for h in pick0] if s == 0 else [(h, 0.3 + 0.01 * h) for h in range(0, H, 3)])
    vis = _visits(sset.species[0])
    order = sorted(pick0)                                                    # bit k of the compact masks = the k-th selected haplotype in ascending index
    assert (vis[:, order[:64]].any(axis=1) & vis[:, order[64:]].any(axis=1)).any()   # some node's M(v) has bits in both words
    assert order != pick0 and len(set(w.values())) == 80
    return sel


def test_fit_wide_species(eng, set_opt):
    import synthdata as synth
    sset = synth.make_set(923, 2, 100, 8000, 12000)
    bases = _coverage(eng, sset)
    sel = wide_case(sset)
    exp = fit(sset.species, *sel, bases)
    assert exp[0][:80, 0, 3].all() and exp[1][0, 2, 0] > 0                   # every entry predicts bases; orphans
    check_identities(*exp)
    _check(_both_routes(eng, set_opt, sel), exp)


@pytest.fixture(scope="module")
def chunked():
    import synthdata as synth
    return synth.make_set(924, 4, 5, 20000, 30000, present_frac=0.6, single_strain_every=2)


def test_fit_single_strain_chunk_graphs(eng, chunked, set_opt):
    """K = 1: all == private == explained; a single strain that walks every node of its species: explained == total, nothing orphan"""
    sset = chunked
    assert [g.n_paths for g in sset.species] == [5, 1, 5, 1]
    bases = _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: [(0, 2.5)] if H == 1 else ([(2, 1.75)] if s == 0 else [(h, 0.5 + 0.25 * h) for h in range(H)]))
    got = _both_routes(eng, set_opt, sel)
    _check(got, fit(sset.species, *sel, bases))
    hap, sp = got
    for s, c in ((0, 0), (1, 1), (3, 7)):                                    # the three species with one selected strain, and its entry
        assert int(sel[0][s + 1] - sel[0][s]) == 1
        assert np.array_equal(hap[c, 0], hap[c, 1]) and np.array_equal(hap[c, 0], sp[s, 1])
    for s, c in ((1, 1), (3, 7)):
        g = sset.species[s]
        assert len(np.unique(g.path_nodes)) == g.n_nodes                     # the strain walks every node
        assert np.array_equal(sp[s, 1], sp[s, 0]) and not sp[s, 2].any() and sp[s, 0, 3] > 0
    assert sp[0, 2, 0] > 0 and sp[0, 1, 0] < sp[0, 0, 0]                     # one strain of five leaves orphans
    check_identities(hap, sp)


def test_fit_long_reads(eng):
    """long reads on 300-kb genomes: many chunks add into the same counters, more aligned bases than the genome is long"""
    import synthdata as synth
    sset = synth.make_set(925, 2, 6, 400, 300000, long_reads=True)
    bases = _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: [(1, 0.8), (4, 0.05), (2, 1.9)] if s == 0 else [(h, 0.4 * (h + 1)) for h in range(H)])
    got = eng.strain_fit(*sel)
    _check(got, fit(sset.species, *sel, bases))
    assert all(g.n_nodes > 8 * CHUNK for g in sset.species)                  # many chunks add into the same counters
    assert np.any(got[0][:, 0, 2] > got[0][:, 0, 1]) and np.all(got[1][:, 0, 2] > got[1][:, 0, 1])
    check_identities(*got)


def test_fit_ties_to_the_evidence_call(eng, narrow):
    """on the same resident coverage: {n_nodes, len, bases} of all, private, total and orphan are columns {0, 1, 3} of the evidence call; all weights
    zero: nothing expected; every identity of the contract on the device's own output"""
    sset = narrow
    _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: [(5, 0.6), (1, 2.0), (3, 1e-3)] if s == 1 else ([(3, 1.25)] if s == 0 else [(h, 0.1 * h) for h in range(H)]))
    hap, sp = eng.strain_fit(*sel)
    ev_hap, ev_sp = eng.strain_evidence(sel[0], sel[1])
    assert np.array_equal(hap[:, :, :3], ev_hap[:, :, [0, 1, 3]])
    assert np.array_equal(sp[:, 0, :3], ev_sp[:, 0][:, [0, 1, 3]]) and np.array_equal(sp[:, 2, :3], ev_sp[:, 1][:, [0, 1, 3]])
    assert hap[:, 0, 3].sum() > 0 and hap[:, 0, 4].sum() > 0
    check_identities(hap, sp)
    hap0, sp0 = eng.strain_fit(sel[0], sel[1], np.zeros(len(sel[1])))
    assert not hap0[:, :, 3].any() and not hap0[:, :, 5:].any() and not sp0[:, :, 3].any() and not sp0[:, :, 5:].any()
    assert np.array_equal(hap0[:, :, :3], hap[:, :, :3]) and np.array_equal(sp0[:, :, :3], sp[:, :, :3])
    check_identities(hap0, sp0)


def _raw(eng, sel_off, sel_hap, sel_w, n_species=None, fill=77, null_w=False):
    """the C call as it is: (rc, hap, species); the arrays are pre-filled with `fill`"""
    from pantax_amd import _ffi
    so, sh = np.ascontiguousarray(sel_off, dtype=np.uint64), np.ascontiguousarray(sel_hap, dtype=np.uint32)
    sw = np.ascontiguousarray(sel_w, dtype=np.float64)
    cs = _ffi.FitSet(eng.S if n_species is None else n_species, so.ctypes.data, sh.ctypes.data if len(sh) else None, sw.ctypes.data if len(sw) and not null_w else None)
    hap = np.full((max(len(sh), 1), 2, 8), fill, dtype=np.uint64)
    sp = np.full((eng.S, 3, 8), fill, dtype=np.uint64)
    rc = eng.lib.pantax_hip_strain_fit(eng.ctx, eng.db, C.byref(cs), _ffi.p(hap), _ffi.p(sp))
    return rc, hap[:len(sh)], sp


def test_fit_state_and_arguments(eng, narrow):
    from pantax_amd._ffi import PantaxHipError
    sset = narrow
    eng._fit_resident = None
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    sel = _selection(sset.species, lambda s, H: [(4, 0.75), (1, 1.5)] if s == 1 else ([(H - 1, 2.0)] if s == 0 else []))
    assert _raw(eng, *sel)[0] == E_STATE                                     # no coverage pass yet
    bases, _, _, _ = eng.get_node_abundances()
    exp = fit(sset.species, *sel, bases)
    rc, hap, sp = _raw(eng, *sel)
    assert rc == 0
    _check((hap, sp), exp)
    # refused arguments: nothing is written
    for args, kw in ((([0, 0, 2, 2], [3, 3], [1.0, 1.0]), {}),               # a haplotype twice within a species
                     (([0, 1, 1, 1], [sset.species[0].n_paths], [1.0]), {}),  # index = n_paths
                     ((sel[0][:-1], sel[1], sel[2]), {"n_species": eng.S - 1}),
                     ((sel[0], sel[1], [0.75, np.nan, 2.0]), {}),            # a weight that is no number,
                     ((sel[0], sel[1], [0.75, 1.5, -1e-300]), {}),           # negative,
                     ((sel[0], sel[1], [np.inf, 1.5, 2.0]), {}),             # infinite,
                     ((sel[0], sel[1], sel[2]), {"null_w": True})):          # or missing
        rc, hap, sp = _raw(eng, *args, **kw)
        assert rc == E_INVALID and np.all(hap == 77) and np.all(sp == 77)
    # nothing selected: every node of every species is an orphan
    rc, hap, sp = _raw(eng, [0, 0, 0, 0], [], [])
    assert rc == 0 and len(hap) == 0 and np.array_equal(sp[:, 0], sp[:, 2]) and not sp[:, 1].any()
    assert sp[:, 0, 0].tolist() == [g.n_nodes for g in sset.species] and np.array_equal(sp[:, 0, :3], exp[1][:, 0, :3])
    # a resident step may zero the arena: refused behind it, fine again behind the next stage call
    eng.profile_step(sset.avg_len())
    with pytest.raises(PantaxHipError) as e:
        eng.strain_fit(*sel)
    assert e.value.code == E_STATE and "resident step" in str(e.value)
    assert _raw(eng, *sel)[0] == E_STATE
    eng.get_node_abundances(fetch=False)
    _check(eng.strain_fit(*sel), exp)


# ---- the file seam -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world(tmp_path_factory):
    yield from seam_world(tmp_path_factory, "pantax_fit", 32, 4, 5, 30000, 30000, present_frac=0.4, single_strain_every=4, with_ids=True)


HEADER = ["species_taxid", "strain_taxid", "genome_ID", "class", "n_nodes", "len", "bases", "expected", "excess", "deficit", "blind_nodes", "blind_expected",
          "fit", "predicted_coverage"]


def test_profile_seam_strain_fit(world, set_opt, capfd):
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng = world
    _profile(eng, db, root / "wd_plain", gaf)
    wd = root / "wd_fit"
    _profile(eng, db, wd, gaf, strain_fit_file=str(wd / "fit.tsv"))
    for f in ("species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt"):   # the option changes none of the tables
        assert open(wd / f, "rb").read() == open(root / "wd_plain" / f, "rb").read()
    assert not os.path.exists(root / "wd_plain" / "fit.tsv")
    rows = _lines(wd / "fit.tsv")
    assert rows[0] == HEADER and all(len(r) == len(HEADER) for r in rows)
    rows = rows[1:]
    table = _lines(wd / "strain_abundance.txt")[1:]
    n_str = len(table)
    assert n_str >= 2 and len({tuple(r[:3]) for r in table}) == n_str
    # strain rows first: all, then private, per row of the table in its order, with the table's predicted_coverage, bit for bit
    assert [(tuple(r[:3]), r[3]) for r in rows[:2 * n_str]] == [(tuple(t[:3]), cls) for t in table for cls in ("all", "private")]
    assert all(np.float64(rows[2 * i + k][13]) == np.float64(table[i][3]) for i in range(n_str) for k in (0, 1))
    sp_rows = rows[2 * n_str:]
    assert all(r[1] == "-" and r[2] == "-" and r[3] in ("total", "explained", "orphan") for r in sp_rows)
    # the stage outputs of the same sample for the table's rows and weights
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
    sel_w = np.array([np.float64(table[i][3]) for p in picked for _, i in p], dtype=np.float64)
    hap, sp = eng.strain_fit(sel_off, sel_hap, sel_w)
    entry_of_row = {i: int(sel_off[s]) + k for s, p in enumerate(picked) for k, (_, i) in enumerate(p)}
    ints = lambda r: [int(x) for x in r[4:12]]
    for i in range(n_str):
        assert ints(rows[2 * i]) == hap[entry_of_row[i], 0].tolist() and ints(rows[2 * i + 1]) == hap[entry_of_row[i], 1].tolist()
    # species rows: every species that went through the strain step, in the run's order; explained only where the species has rows
    seq = []
    for r in sp_rows:
        if not seq or seq[-1] != r[0]:
            seq.append(r[0])
    idx = [names.index(x) for x in seq]
    sp_table = [r[0] for r in _lines(wd / "species_abundance.txt")[1:]]          # the run takes the selected species in the order of the species table
    assert len(set(seq)) == len(seq) >= 2 and seq == [x for x in sp_table if x in set(seq)] and {t[0] for t in table} <= set(seq)
    at = 0
    for s in idx:
        classes = [("total", 0)] + ([("explained", 1)] if picked[s] else []) + [("orphan", 2)]
        mine = sp_rows[at:at + len(classes)]
        at += len(classes)
        assert [r[3] for r in mine] == [c for c, _ in classes] and all(r[0] == names[s] for r in mine)
        for r, (_, k) in zip(mine, classes):
            assert ints(r) == sp[s, k].tolist()
        assert mine[0][13] == "-" and mine[-1][13] == "-"
        if picked[s]:
            pc = np.float64(0.0)
            for _, i in picked[s]:                                           # ascending haplotype index
                pc += np.float64(table[i][3])
            assert np.float64(mine[1][13]) == pc
    assert at == len(sp_rows)
    for r in rows:                                                           # fit parses back bit for bit; "-" where nothing is aligned or expected
        q = [int(x) for x in r[4:12]]
        if q[2] + q[3]:
            assert np.float64(r[12]) == np.float64(1.0) - np.float64(q[4] + q[5]) / np.float64(q[2] + q[3])
        else:
            assert r[12] == "-"
    assert any(r[3] == "private" and int(r[4]) > 0 for r in rows) and any(r[3] == "explained" and int(r[7]) > 0 for r in rows)
    assert any(int(r[8]) > 0 for r in rows) and any(int(r[9]) > 0 for r in rows) and any(int(r[10]) > 0 for r in rows)
    # the path that cuts the species into groups: the same file from more than one group
    wg = root / "wd_fit_groups"
    set_opt(eng, "db_path_steps_max", 1)
    try:
        _profile(eng, db, wg, gaf, strain_fit_file=str(wg / "fit.tsv"))
    finally:
        set_opt(eng, "db_path_steps_max", None)
    assert open(wg / "fit.tsv", "rb").read() == open(wd / "fit.tsv", "rb").read()
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_fit_cli"
    wc.mkdir()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0",
                        "--strain-fit", str(wc / "fit.tsv")], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc / "fit.tsv", "rb").read() == open(wd / "fit.tsv", "rb").read()
    # the strain-only resume writes the same file; a run without a strain step writes nothing and says so
    wr = root / "wd_fit_resume"
    _profile(eng, db, wr, gaf, species=True, strain=False, out_binning_file=str(wr / "reads_classification.tsv"), strain_fit_file=str(wr / "fit_species.tsv"))
    assert not os.path.exists(wr / "fit_species.tsv")
    _profile(eng, db, wr, gaf, species=False, strain=True, strain_fit_file=str(wr / "fit.tsv"))
    assert open(wr / "fit.tsv", "rb").read() == open(wd / "fit.tsv", "rb").read()
    capfd.readouterr()
    _profile(eng, db, wr, gaf, species=True, strain=True, strain_fit_file=str(wr / "fit_again.tsv"))
    assert not os.path.exists(wr / "fit_again.tsv") and "no strain step" in capfd.readouterr().err
    # several ranks
    for rank in range(2):
        wn = root / ("wd_fit_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, strain_fit_file=str(wn / "fit.tsv"))
        assert e.value.code == E_INVALID and "strain_fit_file" in str(e.value)
        assert not os.path.exists(wn / "fit.tsv") and not os.path.exists(wn / "species_abundance.txt")
