"""GPU tests of the own-node windows of a strain and the replication index report on top of them (pantax_hip_strain_growth, --strain-growth).  The expected
values come from the numpy restatement of the contract in tests/growth_ref.py (pinned by tests/test_growth_ref.py on cases done by hand), applied to the
bases_per_node that get_node_abundances hands out -- the parity tests pin those against the oracle.  Everything the stage call returns is an integer: every
comparison is np.array_equal.  Every test asserts, from its own set, that the shape it is about is there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import growth_ref as ref
from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile, seam_world

pytestmark = pytest.mark.gpu

TILE = 1024        # the kernels cut the walks at the multiples of 1024 global path positions; a lane holds 16 consecutive positions
E_INVALID, E_LIMIT, E_STATE = -1, -4, -7
MASK, ACCUM = "read_strain_mask_kernel", "growth_accum_kernel"


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _coverage(eng, sset):
    """the set resident with a coverage result of the stage kind -> bases_per_node; computed once per set"""
    if getattr(eng, "_gr_resident", None) is not sset:
        eng.upload_db(sset.species)
        eng.upload_packed(sset.reads)
        eng.rcls_profile(want_species=False)
        eng.trio_nodes_info()
        bases, _, _, _ = eng.get_node_abundances()
        sset._gr_bases = np.array(bases, copy=True)
        eng._gr_resident = sset
    return sset._gr_bases


def _selection(species, pick):
    off, hp = [0], []
    for s, g in enumerate(species):
        hp += list(pick(s, g.n_paths))
        off.append(len(hp))
    return np.array(off, dtype=np.uint64), np.array(hp, dtype=np.uint32)


def _check(got, exp):
    assert len(got) == len(exp) == 5
    for a, b in zip(got, exp):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _walk_span(species, sel_off, sel_hap):
    """(first global path position, steps) of every selected walk, in the order of sel_hap"""
    base = np.concatenate([[0], np.cumsum([int(g.path_off[-1]) for g in species])])
    return [(int(base[s] + g.path_off[int(sel_hap[c])]), int(g.path_off[int(sel_hap[c]) + 1] - g.path_off[int(sel_hap[c])]))
            for s, g in enumerate(species) for c in range(int(sel_off[s]), int(sel_off[s + 1]))]


@pytest.fixture(scope="module")
def main_set():
    import synthdata as synth
    return synth.make_set(917, 3, 6, 2000, 60000)


@pytest.fixture(scope="module")
def wide_set():
    """a species of 70 haplotypes (two mask words, route 2 whatever the option) and one of 6, cut into short nodes"""
    import synthdata as synth
    from types import SimpleNamespace
    rng = np.random.default_rng(20261101)
    species, start = [], 1
    for s, h in enumerate((70, 6)):
        g = synth.make_species(rng, str(1000 + s), h, 8000, start, "GCF_%06d" % (s + 1), mean_len=8, present_frac=0.3)
        species.append(g)
        start = g.range_end + 1
    return SimpleNamespace(species=species, reads=synth.make_reads(rng, species, 8000))


@pytest.mark.parametrize("W", [1, 100, 5000, 10 ** 9])
def test_growth_all_haplotypes(eng, main_set, W):
    """every haplotype selected: windows inside a lane, over lanes and over tiles; own and shared steps side by side"""
    sset = main_set
    bases = _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: range(H))
    exp = ref.windows(sset.species, *sel, W, bases)
    spans = _walk_span(sset.species, *sel)
    assert any(p % 16 for p, _ in spans) and any(p % TILE for p, _ in spans)       # walks that begin inside a lane and inside a tile
    assert all(n > 2 * TILE for _, n in spans)                                      # every walk crosses tile borders ...
    n_win = np.diff(exp[0].astype(np.int64))
    n_steps = np.array([n for _, n in spans])
    if W == 10 ** 9:
        assert n_win.tolist() == [1] * len(spans)                                   # ... and so does the one window of every strain
    elif W == 5000:
        assert np.all(n_steps / n_win > 64 * 16 / 8) and np.all(n_win > 8)          # windows of hundreds of steps: over lanes, some over a tile border
    elif W == 100:
        assert int((exp[2] == 0).sum()) > 100 and np.all(n_steps / n_win < 16)      # windows no node starts in; several windows inside a lane
    else:
        assert np.array_equal(n_win, [int(sset.species[s].node_len[sset.species[s].path_nodes[int(sset.species[s].path_off[h]):int(sset.species[s].path_off[h + 1])]].sum())
                                      for s in range(3) for h in range(6)])         # one window a base: every step a window of its own
    total_steps = int(n_steps.sum())
    assert 1000 < int(exp[1].sum()) < total_steps // 2 and 0 < int(exp[3].sum()) < int(exp[2].sum())   # own steps and steps that are not
    assert int(exp[4].sum()) > 0
    _check(eng.strain_growth(*sel, W), exp)


def test_growth_one_haplotype_is_the_track(eng, main_set):
    """one selected haplotype a species: every step is own, and the windows are those of the coverage track -- a cross-check without a reference"""
    sset = main_set
    bases = _coverage(eng, sset)
    for pick in (lambda s, H: [s + 1], lambda s, H: [H - 1] if s != 1 else []):
        sel = _selection(sset.species, pick)
        for W in (100, 5000):
            got = eng.strain_growth(*sel, W)
            tr = eng.strain_cov_track(*sel, W)
            assert np.array_equal(got[0], tr[0]) and np.array_equal(got[1], tr[1]) and np.array_equal(got[2], tr[2]) and np.array_equal(got[3], tr[2])
            assert np.array_equal(got[4], tr[4]) and int(got[4].sum()) > 0 and int(got[1].sum()) > 2 * TILE
            _check(got, ref.windows(sset.species, *sel, W, bases))


def _timed(eng, call):
    eng.timing_enable(True)
    eng.timing_reset()
    try:
        got = call()
        ran = set(eng.timing_get())
    finally:
        eng.timing_enable(False)
    return got, ran


def test_growth_route_walk_gives_the_same(eng, main_set, set_opt):
    """the default takes the node -> haplotype words built at upload (route 1: no mask pass), growth_route=walk the masks of the selected walks (route 2)"""
    sset = main_set
    bases = _coverage(eng, sset)
    assert all(g.n_paths <= 64 for g in sset.species)                              # route 1 is open to every species of the set
    for pick in (lambda s, H: range(H), lambda s, H: [4, 1, 3] if s == 0 else ([] if s == 1 else [H - 1, 0])):
        sel = _selection(sset.species, pick)
        by_node, ran1 = _timed(eng, lambda: eng.strain_growth(*sel, 100))
        set_opt(eng, "growth_route", "walk")
        by_walk, ran2 = _timed(eng, lambda: eng.strain_growth(*sel, 100))
        set_opt(eng, "growth_route", None)
        assert ACCUM in ran1 and ACCUM in ran2 and MASK not in ran1 and MASK in ran2, (sorted(ran1), sorted(ran2))
        _check(by_walk, by_node)
        _check(by_node, ref.windows(sset.species, *sel, 100, bases))
        assert 0 < int(by_node[1].sum())


def test_growth_wide_species_second_word(eng, wide_set):
    """70 selected haplotypes of one species: two mask words a node, own bits in the second; in any order of the selection"""
    sset = wide_set
    bases = _coverage(eng, sset)
    assert [g.n_paths for g in sset.species] == [70, 6]
    sel = _selection(sset.species, lambda s, H: range(H))
    exp = ref.windows(sset.species, *sel, 100, bases)
    own_bases = np.array([int(exp[4][int(exp[0][c]):int(exp[0][c + 1])].sum()) for c in range(70)])
    assert (own_bases > 0).sum() >= 6                                              # strains with reads on nodes of their own ...
    order = np.argsort(own_bases > 0, kind="stable")                               # ... go to the end of the second selection: behind bit 64
    for pick in (lambda s, H: range(H), lambda s, H: order if s == 0 else [5, 0]):
        sel = _selection(sset.species, pick)
        exp = ref.windows(sset.species, *sel, 100, bases)
        own = np.array([int(exp[1][int(exp[0][c]):int(exp[0][c + 1])].sum()) for c in range(70)])
        assert int(sel[0][1]) == 70 > 64 and (own[64:] > 0).sum() >= 4 and (own[:64] > 0).sum() >= 40        # own steps behind bits of either word
        if pick(0, 70) is order:
            assert np.all(exp[4][int(exp[0][64]):int(exp[0][70])].sum() > 0) and int(exp[4][:int(exp[0][64])].sum()) > 0   # ... that carry bases
        got, ran = _timed(eng, lambda: eng.strain_growth(*sel, 100))
        assert MASK in ran and ACCUM in ran                                                                  # more than 64 haplotypes: route 2 whatever the option
        _check(got, exp)
    few = _selection(sset.species, lambda s, H: [69, 3] if s == 0 else [])                                   # two of the 70: one word, bits 0 and 1
    _check(eng.strain_growth(*few, 7), ref.windows(sset.species, *few, 7, bases))


def test_growth_selections(eng, main_set):
    """a selection in non-ascending haplotype order, a species without a selection, an empty selection; what is own depends on the selection"""
    sset = main_set
    bases = _coverage(eng, sset)
    a = _selection(sset.species, lambda s, H: [4, 1, 3] if s == 0 else ([] if s == 1 else [H - 1, 0]))
    got_a = eng.strain_growth(*a, 500)
    _check(got_a, ref.windows(sset.species, *a, 500, bases))
    b = _selection(sset.species, lambda s, H: [1, 4] if s == 0 else [])
    got_b = eng.strain_growth(*b, 500)
    _check(got_b, ref.windows(sset.species, *b, 500, bases))
    lo, hi = int(got_a[0][1]), int(got_a[0][2])                                    # haplotype 1 of species 0: entry 1 of a, entry 0 of b
    assert hi - lo == int(got_b[0][1]) > 0 and np.array_equal(got_a[2][lo:hi], got_b[2][:hi - lo])          # len is the walk's ...
    assert int(got_a[1][lo:hi].sum()) < int(got_b[1][:hi - lo].sum())              # ... own grows when haplotype 3 leaves the selection
    none = eng.strain_growth(np.zeros(eng.S + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), 500)
    assert none[0].tolist() == [0] and all(len(x) == 0 for x in none[1:])


def _raw(eng, sel_off, sel_hap, W, cap, n_species=None, fill=77):
    """the C call as it is: (rc, win_off, n_own, len, len_own, bases_own); the four arrays hold `cap` entries of `fill`"""
    from pantax_amd import _ffi
    so, sh = np.ascontiguousarray(sel_off, dtype=np.uint64), np.ascontiguousarray(sel_hap, dtype=np.uint32)
    cs = _ffi.CovTrackSet(eng.S if n_species is None else n_species, so.ctypes.data, sh.ctypes.data if len(sh) else None, int(W))
    win_off = np.full(len(sh) + 1, 0xABCD, dtype=np.uint64)
    outs = [np.full(max(cap, 1), fill, dtype=dt) for dt in (np.uint32, np.uint64, np.uint64, np.uint64)]
    rc = eng.lib.pantax_hip_strain_growth(eng.ctx, eng.db, C.byref(cs), _ffi.p(win_off), cap, *[_ffi.p(o) for o in outs])
    return (rc, win_off, *outs)


def test_growth_sizing_and_state(eng, main_set):
    from pantax_amd._ffi import PantaxHipError
    sset = main_set
    eng._gr_resident = None
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    sel = _selection(sset.species, lambda s, H: [4, 1] if s == 1 else ([H - 1] if s == 0 else []))
    assert _raw(eng, *sel, 500, 0)[0] == E_STATE                                   # no coverage pass yet
    bases, _, _, _ = eng.get_node_abundances()
    exp = ref.windows(sset.species, *sel, 500, bases)
    total = int(exp[0][-1])
    assert total > 100
    for cap in (0, total - 1):                                                     # sizing: the prefix is written, the arrays are not touched
        r = _raw(eng, *sel, 500, cap)
        assert r[0] == E_LIMIT and np.array_equal(r[1], exp[0])
        assert all(np.all(o == 77) for o in r[2:])
    r = _raw(eng, *sel, 500, total)                                                # exact
    assert r[0] == 0
    _check(r[1:], exp)
    # refused arguments
    assert _raw(eng, *sel, 0, total)[0] == E_INVALID                               # W = 0
    assert _raw(eng, [0, 0, 2, 2], [3, 3], 500, total)[0] == E_INVALID             # a haplotype twice within a species
    assert _raw(eng, [0, 1, 1, 1], [sset.species[0].n_paths], 500, total)[0] == E_INVALID   # index = n_paths
    assert _raw(eng, sel[0][:-1], sel[1], 500, total, n_species=eng.S - 1)[0] == E_INVALID
    # nothing selected is fine
    r = _raw(eng, [0, 0, 0, 0], [], 500, 0)
    assert r[0] == 0 and r[1].tolist() == [0]
    # a resident step may zero the coverage arena: refused behind it, fine again behind the next stage call
    eng.profile_step(sset.avg_len())
    with pytest.raises(PantaxHipError) as e:
        eng.strain_growth(*sel, 500)
    assert e.value.code == E_STATE and "resident step" in str(e.value)
    eng.get_node_abundances(fetch=False)
    _check(eng.strain_growth(*sel, 500), exp)


# ---- the file seam -----------------------------------------------------------------------------------------------------------

HEADER = ["species_taxid", "strain_taxid", "genome_ID", "window", "n_windows", "n_kept", "n_zero", "n_fit", "own_len", "own_fraction", "median_depth", "slope",
          "intercept", "r2", "index", "status", "predicted_coverage"]
INT_COLS = {"n_kept": 5, "n_zero": 6, "n_fit": 7, "own_len": 8}
FLOAT_COLS = {"median_depth": 10, "slope": 11, "intercept": 12, "r2": 13, "index": 14}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """two species of five strains and two of a single strain (chains of 1024-base nodes, every step its own), deep enough for a fit"""
    yield from seam_world(tmp_path_factory, "pantax_gr", 32, 4, 5, 20000, 30000, present_frac=0.4, single_strain_every=2, with_ids=True)


def _same_rows(sset, db, wd, eng, body, W, own_permille, trim):
    """the report against the stage call of the same sample, the fit reference and the run's strain table -> the statuses"""
    table = _lines(wd / "strain_abundance.txt")[1:]
    assert len(body) == len(table) > 4
    names = [g.name for g in sset.species]
    genome_hap = {r[0]: r[0].split("_ASM")[0] for r in _lines(db / "genomes_info.txt")[1:]}
    picked = [[] for _ in names]                                                   # per species: (haplotype, row of the table)
    for i, t in enumerate(table):
        s = names.index(t[0])
        picked[s].append((sset.species[s].hap_names.index(genome_hap[t[2]]), i))
    off = np.concatenate([[0], np.cumsum([len(pk) for pk in picked])]).astype(np.uint64)
    hp = np.array([h for pk in picked for h, _ in pk], dtype=np.uint32)
    entry_of_row = {i: int(off[s]) + k for s, pk in enumerate(picked) for k, (_, i) in enumerate(pk)}
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    eng.get_node_abundances(fetch=False)
    win_off, _, ln, len_own, bases_own = eng.strain_growth(off, hp, W)
    statuses = []
    for i, (t, row) in enumerate(zip(table, body)):
        e = entry_of_row[i]
        lo, hi = int(win_off[e]), int(win_off[e + 1])
        f = ref.fit(len_own[lo:hi], bases_own[lo:hi], ref.min_own_of(W, own_permille), trim)
        G = int(ln[lo:hi].sum())
        assert len(row) == len(HEADER) and row[:3] == t[:3] and row[3] == str(W) and row[4] == str(hi - lo) and row[15] == f["status"], (row, f)
        for k, c in INT_COLS.items():
            assert row[c] == str(f[k]), (k, row, f)
        for k, c in list(FLOAT_COLS.items()) + [("own_fraction", 9)]:
            want = f["own_len"] / G if k == "own_fraction" else f[k]
            assert abs(float(row[c]) - want) <= 1e-9 * abs(want), (k, row, f)
        assert np.float64(row[16]) == np.float64(t[3])
        statuses.append(f["status"])
    return statuses


@pytest.fixture(scope="module")
def seam_runs(world):
    """the run without the option and the run at W = 200 that the seam tests compare with; made once"""
    sset, root, db, gaf, eng = world
    plain, wd = root / "wd_plain", root / "wd_gr"
    _profile(eng, db, plain, gaf)
    _profile(eng, db, wd, gaf, strain_growth_file=str(wd / "gr.tsv"), strain_growth_window=200)
    return plain, wd, open(wd / "gr.tsv", "rb").read()


def test_profile_seam_strain_growth(world, seam_runs):
    """the report against the stage call and the fit reference; the other outputs of the run are those of a run without the option"""
    sset, root, db, gaf, eng = world
    plain, wd, _ = seam_runs
    for f in ("species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt"):      # the option changes none of the other outputs
        assert open(wd / f, "rb").read() == open(plain / f, "rb").read()
    assert sorted(os.listdir(wd)) == sorted(os.listdir(plain) + ["gr.tsv"])
    rows = _lines(wd / "gr.tsv")
    assert rows[0] == HEADER
    st = _same_rows(sset, db, wd, eng, rows[1:], 200, 500, 100)
    assert "ok" in st and len(set(st)) >= 2, st                                                  # strains with a fit, and strains without one


def test_profile_seam_growth_parameters(world):
    """the defaults (5 000 bases: six windows a strain, too few for a fit), and the three parameters"""
    sset, root, db, gaf, eng = world
    w2 = root / "wd_gr_default"
    _profile(eng, db, w2, gaf, strain_growth_file=str(w2 / "gr.tsv"))
    st2 = _same_rows(sset, db, w2, eng, _lines(w2 / "gr.tsv")[1:], 5000, 500, 100)
    assert set(st2) <= {"few_windows", "empty"}
    w3 = root / "wd_gr_params"
    _profile(eng, db, w3, gaf, strain_growth_file=str(w3 / "gr.tsv"), strain_growth_window=150, strain_growth_min_own=200, strain_growth_trim=30)
    _same_rows(sset, db, w3, eng, _lines(w3 / "gr.tsv")[1:], 150, 200, 30)
    wc = root / "wd_gr_params_cli"                                                                # ... and through the command-line front end
    wc.mkdir()
    r = subprocess.run([os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip"), "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read",
                        "--sample", "0", "--strain-growth", str(wc / "gr.tsv"), "--strain-growth-window", "150", "--strain-growth-min-own", "200", "--strain-growth-trim", "30"],
                       cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc / "gr.tsv", "rb").read() == open(w3 / "gr.tsv", "rb").read()


def test_profile_seam_growth_over_groups(world, seam_runs, set_opt):
    """a run over several groups of species writes the same file as a run over one"""
    sset, root, db, gaf, eng = world
    _, _, full = seam_runs
    wg = root / "wd_gr_groups"
    set_opt(eng, "db_groups", 2)
    _profile(eng, db, wg, gaf, strain_growth_file=str(wg / "gr.tsv"), strain_growth_window=200)
    set_opt(eng, "db_groups", None)
    assert open(wg / "gr.tsv", "rb").read() == full and len(sset.species) >= 2


def test_profile_seam_growth_resume_and_cli(world, seam_runs, capfd):
    sset, root, db, gaf, eng = world
    _, _, full = seam_runs
    # a species-only run writes nothing and says so; the strain-only resume behind it writes the same file
    wr = root / "wd_gr_resume"
    capfd.readouterr()
    _profile(eng, db, wr, gaf, species=True, strain=False, out_binning_file=str(wr / "reads_classification.tsv"), strain_growth_file=str(wr / "gr_species_only.tsv"))
    assert not os.path.exists(wr / "gr_species_only.tsv") and "no strain step" in capfd.readouterr().err
    _profile(eng, db, wr, gaf, species=False, strain=True, strain_growth_file=str(wr / "gr.tsv"), strain_growth_window=200)
    assert open(wr / "gr.tsv", "rb").read() == full
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_gr_cli"
    wc.mkdir()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0", "--strain-growth",
                        str(wc / "gr.tsv"), "--strain-growth-window", "200"], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc / "gr.tsv", "rb").read() == full
    r = subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=120)
    for flag in ("--strain-growth-window", "--strain-growth-min-own", "--strain-growth-trim"):
        assert flag in r.stdout + r.stderr


def test_profile_seam_growth_refusals_and_older_callers(world, seam_runs, monkeypatch):
    from pantax_amd import _ffi
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng = world
    _, wd, _ = seam_runs
    # refused parameters, and several ranks: refused on every rank with the table's wording, before any collective
    wb = root / "wd_gr_bad"
    with pytest.raises(PantaxHipError) as e:
        _profile(eng, db, wb, gaf, strain_growth_file=str(wb / "gr.tsv"), strain_growth_trim=500)
    assert e.value.code == E_INVALID and "strain_growth_trim_permille 500" in str(e.value)
    for rank in range(2):
        wn = root / ("wd_gr_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, strain_growth_file=str(wn / "gr.tsv"))
        assert e.value.code == E_INVALID and "the replication index report (strain_growth_file) needs one rank and an unsharded ingest (world_size 2)" in str(e.value)
        assert not os.path.exists(wn / "gr.tsv")
    # a caller compiled against the header before these fields: its struct ends behind strain_fragments_file, the report reads as off
    real = _ffi.ProfileExt

    class OldExt(real):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.struct_size = 208

    monkeypatch.setattr(_ffi, "ProfileExt", OldExt)
    wold = root / "wd_gr_old"
    _profile(eng, db, wold, gaf, strain_fit_file=str(wold / "fit.tsv"), strain_growth_file=str(wold / "gr.tsv"))
    monkeypatch.setattr(_ffi, "ProfileExt", real)
    assert os.path.exists(wold / "fit.tsv") and not os.path.exists(wold / "gr.tsv")
    assert open(wold / "strain_abundance.txt", "rb").read() == open(wd / "strain_abundance.txt", "rb").read()
