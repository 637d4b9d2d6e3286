"""GPU tests of the per-strain windowed coverage track (pantax_hip_strain_cov_track, --strain-coverage).  The expected values come from the numpy
restatement of the contract in tests/cov_track_ref.py (pinned by tests/test_cov_track_ref.py on a hand-computed case), applied to the bases_per_node
and node_base_cov that get_node_abundances hands out -- the parity tests pin those against the oracle.  Everything is an integer: every comparison
is np.array_equal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile, seam_world
from tests.cov_track_ref import track, walk_windows

pytestmark = pytest.mark.gpu

TILE = 1024        # the kernels cut the walks at the multiples of 1024 global path positions; a lane holds 16 consecutive positions
E_INVALID, E_LIMIT, E_STATE = -1, -4, -7


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _coverage(eng, sset):
    """the set resident with a coverage result of the stage kind -> (bases_per_node, node_base_cov); computed once per set"""
    if getattr(eng, "_ct_resident", None) is not sset:
        eng.upload_db(sset.species)
        eng.upload_packed(sset.reads)
        eng.rcls_profile(want_species=False)
        eng.trio_nodes_info()
        bases, cov, _, _ = eng.get_node_abundances()
        sset._ct_cov = (np.array(bases, copy=True), np.array(cov, copy=True))
        eng._ct_resident = sset
    return sset._ct_cov


def _selection(species, pick):
    off, hp = [0], []
    for s, g in enumerate(species):
        hp += list(pick(s, g.n_paths))
        off.append(len(hp))
    return np.array(off, dtype=np.uint64), np.array(hp, dtype=np.uint32)


def _check(got, exp):
    for a, b in zip(got, exp):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def _walk_spans(species, sel_off, sel_hap):
    """(first, end) global path position of every selected walk, with its species"""
    base = np.concatenate([[0], np.cumsum([int(g.path_off[-1]) for g in species])])
    out = []
    for s, g in enumerate(species):
        for c in range(int(sel_off[s]), int(sel_off[s + 1])):
            h = int(sel_hap[c])
            out.append((s, h, int(base[s] + g.path_off[h]), int(base[s] + g.path_off[h + 1])))
    return out


@pytest.fixture(scope="module")
def narrow():
    import synthdata as synth
    return synth.make_set(911, 3, 6, 20000, 30000, present_frac=0.6)


@pytest.mark.parametrize("W", [1, 37, 1000, 10000, 10 ** 9])
def test_cov_track_windows(eng, narrow, W):
    """all haplotypes of one species, a shuffled subset of the next, none of the last; W = 1: every node its own window, most windows empty;
    W = 1e9: one window per strain"""
    sset = narrow
    bases, cov = _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: range(H) if s == 0 else ([] if s == 2 else [3, 0, 2]))   # any order on the way in
    # the case holds what the kernels can get wrong (computed from the set: a changed generator cannot hollow the test out)
    spans = _walk_spans(sset.species, *sel)
    assert max(e - b for _, _, b, e in spans) > TILE                         # walks longer than one tile
    assert any(e % TILE % 64 and e % 16 for _, _, b, e in spans) and any(b % 16 for _, _, b, e in spans)   # tiles that begin / end inside a wave and a lane
    crossing = 0
    for s, h, b, e in spans:
        g = sset.species[s]
        ln = g.node_len[g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])]]
        w = (np.cumsum(ln) - ln) // 1000
        cuts = np.arange((b // TILE + 1) * TILE, e, TILE) - b                # walk positions that open a tile
        crossing += int((w[cuts] == w[cuts - 1]).sum())
    assert crossing > 0                                                      # windows (of 1000 bases) that span a tile border
    got = eng.strain_cov_track(sel[0], sel[1], W)
    exp = track(sset.species, sel[0], sel[1], W, cov, bases)
    _check(got, exp)
    assert int(got[0][-1]) == len(got[1]) and got[3].sum() > 0 and got[4].sum() > 0
    if W == 1:
        assert (got[1] == 0).sum() > len(got[1]) // 2 and got[1].max() == 1
    if W == 10 ** 9:
        assert np.array_equal(np.diff(got[0].astype(np.int64)), np.ones(9, dtype=np.int64))


@pytest.fixture(scope="module")
def chunked():
    import synthdata as synth
    return synth.make_set(912, 4, 5, 20000, 30000, present_frac=0.6, single_strain_every=2)


@pytest.mark.parametrize("W", [100, 1024])
def test_cov_track_chunk_graphs(eng, chunked, W):
    """single-strain species are chains of 1024-bp nodes: nodes longer than the window (W = 100), windows exactly node-aligned (W = 1024)"""
    sset = chunked
    assert [g.n_paths for g in sset.species] == [5, 1, 5, 1] and int(sset.species[1].node_len[0]) == 1024
    bases, cov = _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: range(H))
    got = eng.strain_cov_track(sel[0], sel[1], W)
    _check(got, track(sset.species, sel[0], sel[1], W, cov, bases))
    c = 5                                                                    # the single strain of species 1
    n = got[1][int(got[0][c]):int(got[0][c + 1])]
    if W == 100:
        assert (n == 0).sum() > 8 * (n == 1).sum() and n.max() == 1          # ten windows per node, nine of them empty
    else:
        assert np.all(n == 1)


def test_cov_track_wide_and_long(eng):
    """many selected walks (80 of a 100-haplotype species), and long reads on a 300-kb genome: deep sums of bases stay exact in u64"""
    import synthdata as synth
    rng = np.random.default_rng(6)
    sset = synth.make_set(913, 2, 100, 8000, 12000, present_frac=0.6)
    bases, cov = _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: rng.permutation(H)[:80].tolist() if s == 0 else range(0, H, 3))
    for W in (500, 10 ** 9):
        _check(eng.strain_cov_track(sel[0], sel[1], W), track(sset.species, sel[0], sel[1], W, cov, bases))
    sset = synth.make_set(914, 2, 6, 400, 300000, long_reads=True, present_frac=0.6)
    bases, cov = _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: range(H))
    for W in (10000, 10 ** 9):
        got = eng.strain_cov_track(sel[0], sel[1], W)
        _check(got, track(sset.species, sel[0], sel[1], W, cov, bases))
    assert len(got[1]) == 12 and int(got[4].max()) > int(got[2].max())       # one window per strain, more aligned bases than the genome is long


def _raw(eng, sel_off, sel_hap, W, cap, n_species=None, fill=77):
    """the C call as it is: (rc, win_off, n_nodes, len, covered, bases); the four arrays hold `cap` entries of `fill`"""
    from pantax_amd import _ffi
    so, sh = np.ascontiguousarray(sel_off, dtype=np.uint64), np.ascontiguousarray(sel_hap, dtype=np.uint32)
    cs = _ffi.CovTrackSet(eng.S if n_species is None else n_species, so.ctypes.data, sh.ctypes.data if len(sh) else None, int(W))
    win_off = np.full(len(sh) + 1, 0xABCD, dtype=np.uint64)
    n = np.full(max(cap, 1), fill, dtype=np.uint32)
    outs = [np.full(max(cap, 1), fill, dtype=np.uint64) for _ in range(3)]
    rc = eng.lib.pantax_hip_strain_cov_track(eng.ctx, eng.db, C.byref(cs), _ffi.p(win_off), cap, _ffi.p(n), *[_ffi.p(o) for o in outs])
    return (rc, win_off, n, *outs)


def test_cov_track_sizing_and_state(eng, narrow):
    from pantax_amd._ffi import PantaxHipError
    sset = narrow
    eng._ct_resident = None
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    sel = _selection(sset.species, lambda s, H: [4, 1] if s == 1 else ([H - 1] if s == 0 else []))
    W = 700
    assert _raw(eng, sel[0], sel[1], W, 0)[0] == E_STATE                     # no coverage pass yet
    bases, cov, _, _ = eng.get_node_abundances()
    exp = track(sset.species, sel[0], sel[1], W, cov, bases)
    total = int(exp[0][-1])
    rc, win_off, n, ln, cv, bs = _raw(eng, sel[0], sel[1], W, 0)             # sizing: the prefix is written, nothing else
    assert rc == E_LIMIT and np.array_equal(win_off, exp[0]) and n[0] == ln[0] == cv[0] == bs[0] == 77
    rc, win_off, n, ln, cv, bs = _raw(eng, sel[0], sel[1], W, total - 1)
    assert rc == E_LIMIT and np.array_equal(win_off, exp[0]) and np.all(n == 77) and np.all(ln == 77) and np.all(cv == 77) and np.all(bs == 77)
    rc, win_off, n, ln, cv, bs = _raw(eng, sel[0], sel[1], W, total)         # exact
    assert rc == 0
    _check((win_off, n, ln, cv, bs), exp)
    # refused arguments
    assert _raw(eng, sel[0], sel[1], 0, total)[0] == E_INVALID
    assert _raw(eng, [0, 0, 2, 2], [3, 3], W, total)[0] == E_INVALID         # a haplotype twice within a species
    assert _raw(eng, [0, 1, 1, 1], [sset.species[0].n_paths], W, total)[0] == E_INVALID   # index = n_paths
    assert _raw(eng, sel[0][:-1], sel[1], W, total, n_species=eng.S - 1)[0] == E_INVALID
    # nothing selected, and a species without selected haplotypes, are fine
    rc, win_off = _raw(eng, [0, 0, 0, 0], [], W, 0)[:2]
    assert rc == 0 and win_off.tolist() == [0]
    # a resident step keeps no node_base_cov and may zero the arena: refused behind it, fine again behind the next stage call
    eng.profile_step(sset.avg_len())
    with pytest.raises(PantaxHipError) as e:
        eng.strain_cov_track(sel[0], sel[1], W)
    assert e.value.code == E_STATE and "resident step" in str(e.value)
    eng.get_node_abundances(fetch=False)
    _check(eng.strain_cov_track(sel[0], sel[1], W), exp)


# ---- the file seam -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world(tmp_path_factory):
    yield from seam_world(tmp_path_factory, "pantax_ct", 32, 4, 5, 30000, 30000, present_frac=0.4, single_strain_every=4, with_ids=True)


def test_profile_seam_strain_coverage(world, set_opt, capfd):
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng = world
    W = 500
    _profile(eng, db, root / "wd_plain", gaf)
    wd = root / "wd_ct"
    _profile(eng, db, wd, gaf, strain_coverage_file=str(wd / "cov.tsv"), strain_coverage_window=W)
    for f in ("species_abundance.txt", "strain_abundance.txt"):              # the option changes none of the tables
        assert open(wd / f, "rb").read() == open(root / "wd_plain" / f, "rb").read()
    assert not os.path.exists(root / "wd_plain" / "cov.tsv")
    rows = _lines(wd / "cov.tsv")
    assert rows[0] == ["species_taxid", "strain_taxid", "genome_ID", "start", "end", "n_nodes", "len", "covered", "bases", "depth", "breadth"]
    rows = rows[1:]
    table = [tuple(r[:3]) for r in _lines(wd / "strain_abundance.txt")[1:]]
    order = []
    for r in rows:
        if not order or order[-1] != tuple(r[:3]):
            order.append(tuple(r[:3]))
    assert order == table and len(set(table)) == len(table) >= 2             # the strains of the table, in its order, each in one block
    # the stage outputs of the same sample, and the restatement on them
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    bases, cov, _, _ = eng.get_node_abundances()
    node_off = np.concatenate([[0], np.cumsum([g.n_nodes for g in sset.species])])
    node_len = np.concatenate([g.node_len for g in sset.species])
    names = [g.name for g in sset.species]
    genome_hap = {r[0]: r[0].split("_ASM")[0] for r in _lines(db / "genomes_info.txt")[1:]}
    n_cut = 0
    for key in table:
        s = names.index(key[0])
        g = sset.species[s]
        h = g.hap_names.index(genome_hap[key[2]])
        walk = g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])].astype(np.int64) + node_off[s]
        n, ln, cv, bs = walk_windows(walk, node_len, cov, bases, W)
        G = int(ln.sum())
        keep = np.nonzero(ln)[0]                                             # windows in which no node starts are not written
        mine = [r for r in rows if tuple(r[:3]) == key]
        assert [int(r[3]) for r in mine] == (keep * W).tolist()
        assert [int(r[4]) for r in mine] == [min((int(w) + 1) * W, G) for w in keep]
        assert [[int(x) for x in r[5:9]] for r in mine] == [[int(n[w]), int(ln[w]), int(cv[w]), int(bs[w])] for w in keep]
        if ln[-1]:                                                           # the last window is written: it ends where the genome ends
            assert int(mine[-1][4]) == G
            n_cut += G % W != 0
        assert sum(int(r[4]) - int(r[3]) for r in mine) == G - sum(min(W, G - int(w) * W) for w in np.nonzero(ln == 0)[0])
        for r in mine:                                                       # the two ratios parse back bit for bit
            assert np.float64(r[9]) == np.float64(int(r[8])) / np.float64(int(r[6])) and np.float64(r[10]) == np.float64(int(r[7])) / np.float64(int(r[6]))
    assert n_cut > 0 and any(int(r[8]) > 0 for r in rows)
    # the path that cuts the species into groups: the same file from more than one group
    wg = root / "wd_ct_groups"
    set_opt(eng, "db_path_steps_max", 1)
    try:
        _profile(eng, db, wg, gaf, strain_coverage_file=str(wg / "cov.tsv"), strain_coverage_window=W)
    finally:
        set_opt(eng, "db_path_steps_max", None)
    assert open(wg / "cov.tsv", "rb").read() == open(wd / "cov.tsv", "rb").read()
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_ct_cli"
    wc.mkdir()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0",
                        "--strain-coverage", str(wc / "cov.tsv"), "--strain-coverage-window", str(W)], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc / "cov.tsv", "rb").read() == open(wd / "cov.tsv", "rb").read()
    # the strain-only resume writes the same file; a run without a strain step writes nothing and says so
    wr = root / "wd_ct_resume"
    _profile(eng, db, wr, gaf, species=True, strain=False, out_binning_file=str(wr / "reads_classification.tsv"), strain_coverage_file=str(wr / "cov_species.tsv"))
    assert not os.path.exists(wr / "cov_species.tsv")
    _profile(eng, db, wr, gaf, species=False, strain=True, strain_coverage_file=str(wr / "cov.tsv"), strain_coverage_window=W)
    assert open(wr / "cov.tsv", "rb").read() == open(wd / "cov.tsv", "rb").read()
    capfd.readouterr()
    _profile(eng, db, wr, gaf, species=True, strain=True, strain_coverage_file=str(wr / "cov_again.tsv"))
    assert not os.path.exists(wr / "cov_again.tsv") and "no strain step" in capfd.readouterr().err
    # the default window, a negative one, several ranks
    wdft = root / "wd_ct_default"
    _profile(eng, db, wdft, gaf, strain_coverage_file=str(wdft / "cov.tsv"))
    assert {int(r[3]) % 10000 for r in _lines(wdft / "cov.tsv")[1:]} == {0}
    with pytest.raises(PantaxHipError) as e:
        _profile(eng, db, root / "wd_ct_neg", gaf, strain_coverage_file=str(root / "wd_ct_neg" / "cov.tsv"), strain_coverage_window=-1)
    assert e.value.code == E_INVALID
    for rank in range(2):
        wn = root / ("wd_ct_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, strain_coverage_file=str(wn / "cov.tsv"))
        assert e.value.code == E_INVALID
        assert not os.path.exists(wn / "cov.tsv") and not os.path.exists(wn / "species_abundance.txt")
