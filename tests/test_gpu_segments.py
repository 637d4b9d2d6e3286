"""GPU tests of the absent and amplified segments along a strain (pantax_hip_strain_segments, --strain-segments).  The expected values come from the numpy
restatement of the contract in tests/segments_ref.py (pinned by tests/test_segments_ref.py on cases done by hand), applied to the bases_per_node and
node_base_cov that get_node_abundances hands out -- the parity tests pin those against the oracle.  Everything is an integer: every comparison is
np.array_equal.  Every test asserts, from its own set, that the shape it is about is there."""
import ctypes as C
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile, seam_world, select_reads
from tests.segments_ref import GAP, PEAK, chain, segments

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
    if getattr(eng, "_sg_resident", None) is not sset:
        eng.upload_db(sset.species)
        eng.upload_packed(sset.reads)
        eng.rcls_profile(want_species=False)
        eng.trio_nodes_info()
        bases, cov, _, _ = eng.get_node_abundances()
        sset._sg_cov = (np.array(bases, copy=True), np.array(cov, copy=True))
        eng._sg_resident = sset
    return sset._sg_cov


def _selection(species, pick):
    off, hp = [0], []
    for s, g in enumerate(species):
        hp += list(pick(s, g.n_paths))
        off.append(len(hp))
    return np.array(off, dtype=np.uint64), np.array(hp, dtype=np.uint32)


def _check(got, exp):
    assert len(got) == len(exp) == 11
    for a, b in zip(got, exp):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _walk_first(species, sel_off, sel_hap):
    """the first global path position of every selected walk, in the order of sel_hap"""
    base = np.concatenate([[0], np.cumsum([int(g.path_off[-1]) for g in species])])
    return np.array([int(base[s] + g.path_off[int(sel_hap[c])]) for s, g in enumerate(species) for c in range(int(sel_off[s]), int(sel_off[s + 1]))], dtype=np.int64)


def _borders(species, sel, ref):
    """per segment of a reference result: how many tile borders it crosses"""
    first = np.repeat(_walk_first(species, *sel), np.diff(ref[0].astype(np.int64)))
    p0 = first + ref[6].astype(np.int64)
    return (p0 + ref[7].astype(np.int64) - 1) // TILE - p0 // TILE


@pytest.fixture(scope="module")
def sparse():
    import synthdata as synth
    return synth.make_set(917, 3, 6, 200, 60000, present_frac=0.35)


@pytest.mark.parametrize("peak_depth", [0, 3])
@pytest.mark.parametrize("min_len", [1, 100, 1000])
def test_segments_sparse_short_reads(eng, sparse, min_len, peak_depth):
    """few short reads on 60-kb genomes: most of every walk is gap, cut by covered nodes -- runs of every length, inside a lane, over lanes, over tiles"""
    sset = sparse
    bases, cov = _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: range(H))
    every = segments(sset.species, *sel, peak_depth, 1, cov, bases)          # all runs: what the case holds
    ln, crossing = every[9], _borders(sset.species, sel, every)
    assert len(ln) > 1000 and (ln < 100).sum() > 100 and ((ln >= 100) & (ln < 1000)).sum() > 100 and (ln >= 1000).sum() > 100
    assert (crossing >= 1).sum() >= 10 and (every[7] == 1).sum() > 10 and (every[7] > 16).sum() > 10   # over a tile border; of one step; longer than a lane
    assert ((every[5] == PEAK).sum() > 10) == (peak_depth == 3)
    # what the oracle gives for this set: 1 635 gap runs, 694 of >= 100 bases and 186 of >= 1 000, the longest 15 547, 39 over a tile border; 34 peak runs at 3
    gap = every[5] == GAP
    assert (int(gap.sum()), int((ln[gap] >= 100).sum()), int((ln[gap] >= 1000).sum()), int(ln.max()), int((crossing >= 1).sum())) == (1635, 694, 186, 15547, 39)
    assert int((every[5] == PEAK).sum()) == (34 if peak_depth == 3 else 0)
    starts = _walk_first(sset.species, *sel)
    assert any(b % 16 for b in starts) and any(b % TILE for b in starts)     # walks that begin inside a lane and inside a tile
    exp = segments(sset.species, *sel, peak_depth, min_len, cov, bases)
    got = eng.strain_segments(*sel, peak_depth, min_len)
    _check(got, exp)
    assert int(got[0][-1]) == len(got[5]) == int((ln >= min_len).sum())
    assert np.array_equal(got[2].sum(axis=0), [(every[5] == GAP).sum(), (every[5] == PEAK).sum()])          # the totals do not depend on min_len
    assert int(got[4].max()) == int(ln.max())


def test_segments_species_without_reads(eng, sparse):
    """the reads binned to species 0 taken out: every walk of that species is ONE gap run through whole-run tiles"""
    from synthdata import PackedReads
    rd = sparse.reads
    eng._sg_resident = None
    eng.upload_db(sparse.species)
    eng.upload_packed(rd)
    sp = np.asarray(eng.rcls_profile()[0])
    keep = np.nonzero(sp != 0)[0]
    so, nid, ps, pe = select_reads(rd, keep)
    old = rd.step_off.astype(np.int64)
    ns = (old[1:] - old[:-1])[keep]
    idx = np.repeat(old[:-1][keep], ns) + (np.arange(int(ns.sum())) - np.repeat(so.astype(np.int64)[:-1], ns))
    sset = SimpleNamespace(species=sparse.species, reads=PackedReads(so.astype(rd.step_off.dtype), nid, rd.strand[idx], ps, pe, rd.qlen[keep], rd.mapq[keep],
                                                                      rd.plen[keep], []))
    assert 0 < len(keep) < rd.n_reads
    bases, cov = _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: range(H))
    for min_len in (1, 1000):
        exp = segments(sset.species, *sel, 3, min_len, cov, bases)
        got = eng.strain_segments(*sel, 3, min_len)
        _check(got, exp)
    H0 = sset.species[0].n_paths
    seg_off, hap_len, n_runs, run_len, run_max = got[:5]
    assert seg_off[:H0 + 1].tolist() == list(range(H0 + 1))                  # one segment per walk of species 0 ...
    assert n_runs[:H0].tolist() == [[1, 0]] * H0 and np.array_equal(run_max[:H0, 0], hap_len[:H0]) and np.array_equal(got[9][:H0], hap_len[:H0])
    assert np.all(got[7][:H0] > 2 * TILE) and np.all(_borders(sset.species, sel, got)[:H0] >= 2)   # ... of about 2 600 steps: whole-run tiles between two borders
    assert n_runs[H0:].sum() > 100                                           # the other species keep their reads


def test_segments_long_reads(eng):
    """long reads on a 300-kb genome: deep nodes, many short peak runs at 10 and long ones at 1; the u64 sums of bases stay exact"""
    import synthdata as synth
    sset = synth.make_set(914, 2, 6, 400, 300000, long_reads=True, present_frac=0.6)
    bases, cov = _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: range(H))
    for peak_depth in (10, 1):
        exp = segments(sset.species, *sel, peak_depth, 1, cov, bases)
        crossing = _borders(sset.species, sel, exp)
        peak = exp[5] == PEAK
        if peak_depth == 10:
            assert peak.sum() > 1000 and (crossing[peak] >= 1).sum() >= 1
        else:
            assert (crossing[peak] >= 2).sum() >= 1                          # a peak run through a whole-run tile
            assert int(exp[10].max()) > int(exp[9].max())                    # more aligned bases in a run than it is long
        _check(eng.strain_segments(*sel, peak_depth, 1), exp)


@pytest.mark.parametrize("min_len", [1024, 1025])
def test_segments_chunk_graphs(eng, min_len):
    """single-strain species are chains of 30 nodes of 1024 bases, shorter than a wave's tile: a run of one node is kept at 1024 and dropped at 1025"""
    import synthdata as synth
    sset = synth.make_set(912, 4, 5, 20000, 30000, present_frac=0.6, single_strain_every=2)
    assert [g.n_paths for g in sset.species] == [5, 1, 5, 1] and int(sset.species[1].node_len[0]) == 1024
    assert all(int(sset.species[s].path_off[1]) == 30 for s in (1, 3))
    bases, cov = _coverage(eng, sset)
    sel = _selection(sset.species, lambda s, H: range(H))
    pd = np.full(12, 3, dtype=np.uint64)
    pd[5] = 16                                                               # the depth at which the single strain of species 1 has peaks of one node
    every = segments(sset.species, *sel, pd, 1, cov, bases)
    for c in (5, 11):                                                        # the two single strains: runs of one node, and in the first longer ones
        ln = every[9][int(every[0][c]):int(every[0][c + 1])]
        assert (ln == 1024).sum() > 0 and ((ln > 1024).sum() > 0 or c == 11)
    exp = segments(sset.species, *sel, pd, min_len, cov, bases)
    got = eng.strain_segments(*sel, pd, min_len)
    _check(got, exp)
    assert ((got[9] == 1024).sum() > 0) == (min_len == 1024)


def test_segments_selections(eng, sparse):
    """any order on the way in, a subset, an empty selection; a haplotype's segments are the same in two selections; a peak_depth per haplotype"""
    sset = sparse
    bases, cov = _coverage(eng, sset)
    a = _selection(sset.species, lambda s, H: [4, 1, 3] if s == 0 else ([] if s == 1 else [H - 1, 0]))
    pd_a = np.array([0, 1, 2, 1, 2 ** 31], dtype=np.uint64)
    got_a = eng.strain_segments(*a, pd_a, 50)
    _check(got_a, segments(sset.species, *a, pd_a, 50, cov, bases))
    assert got_a[2][1, 1] > 10 and got_a[2][3, 1] > 10 and got_a[2][0, 1] == 0 and got_a[2][4, 1] == 0      # peaks at depth 1; none at 0 (off) and at 2^31
    assert segments(sset.species, *a, 1, 50, cov, bases)[2][:, 1].min() > 10                              # ... where every entry has some at 1
    b = _selection(sset.species, lambda s, H: [1] if s == 0 else [])
    got_b = eng.strain_segments(*b, 1, 50)
    _check(got_b, segments(sset.species, *b, 1, 50, cov, bases))
    lo, hi = int(got_a[0][1]), int(got_a[0][2])                              # haplotype 1 of species 0: entry 1 of a, entry 0 of b
    assert hi - lo == int(got_b[0][1]) > 0
    for k in range(5, 11):
        assert np.array_equal(got_a[k][lo:hi], got_b[k])
    assert np.array_equal(got_a[1][1:2], got_b[1]) and np.array_equal(got_a[2][1:2], got_b[2])
    none = eng.strain_segments(np.zeros(eng.S + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), 3, 50)
    assert none[0].tolist() == [0] and all(len(x) == 0 for x in none[1:])


def _raw(eng, sel_off, sel_hap, peak_depth, min_len, cap, n_species=None, fill=77):
    """the C call as it is: (rc, seg_off, hap_len, n_runs, run_len, run_max, class, step, n_steps, start, len, bases); the six arrays hold `cap` entries of `fill`"""
    from pantax_amd import _ffi
    so, sh = np.ascontiguousarray(sel_off, dtype=np.uint64), np.ascontiguousarray(sel_hap, dtype=np.uint32)
    pd = np.ascontiguousarray(np.broadcast_to(np.asarray(peak_depth, dtype=np.uint64), (len(sh),)))
    cs = _ffi.SegmentSet(eng.S if n_species is None else n_species, so.ctypes.data, sh.ctypes.data if len(sh) else None, pd.ctypes.data if len(sh) else None, int(min_len))
    seg_off = np.full(len(sh) + 1, 0xABCD, dtype=np.uint64)
    hap_len = np.full(max(len(sh), 1), 0xABCD, dtype=np.uint64)
    sums = [np.full((max(len(sh), 1), 2), 0xABCD, dtype=np.uint64) for _ in range(3)]
    dts = (np.uint8, np.uint64, np.uint32, np.uint64, np.uint64, np.uint64)
    outs = [np.full(max(cap, 1), fill, dtype=dt) for dt in dts]
    rc = eng.lib.pantax_hip_strain_segments(eng.ctx, eng.db, C.byref(cs), _ffi.p(seg_off), cap, _ffi.p(hap_len), *[_ffi.p(x) for x in sums], *[_ffi.p(o) for o in outs])
    return (rc, seg_off, hap_len[:len(sh)], *[x[:len(sh)] for x in sums], *outs)


def test_segments_sizing_and_state(eng, sparse):
    from pantax_amd._ffi import PantaxHipError
    sset = sparse
    eng._sg_resident = None
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    sel = _selection(sset.species, lambda s, H: [4, 1] if s == 1 else ([H - 1] if s == 0 else []))
    assert _raw(eng, *sel, 3, 100, 0)[0] == E_STATE                          # no coverage pass yet
    bases, cov, _, _ = eng.get_node_abundances()
    exp = segments(sset.species, *sel, 3, 100, cov, bases)
    total = int(exp[0][-1])
    assert total > 10
    for cap in (0, total - 1):                                               # sizing: the prefix and the summaries are written, the arrays are not touched
        r = _raw(eng, *sel, 3, 100, cap)
        assert r[0] == E_LIMIT
        _check(r[1:6] + exp[5:], exp)
        assert all(np.all(o == 77) for o in r[6:])
    r = _raw(eng, *sel, 3, 100, total)                                       # exact
    assert r[0] == 0
    _check(r[1:], exp)
    # refused arguments
    assert _raw(eng, *sel, 3, 0, total)[0] == E_INVALID                      # min_len 0
    assert _raw(eng, *sel, [3, 2 ** 31 + 1, 3], 100, total)[0] == E_INVALID  # a peak_depth above 2^31
    assert _raw(eng, *sel, [3, 2 ** 31, 3], 100, total)[0] == 0
    assert _raw(eng, [0, 0, 2, 2], [3, 3], 3, 100, total)[0] == E_INVALID    # a haplotype twice within a species
    assert _raw(eng, [0, 1, 1, 1], [sset.species[0].n_paths], 3, 100, total)[0] == E_INVALID   # index = n_paths
    assert _raw(eng, sel[0][:-1], sel[1], 3, 100, total, n_species=eng.S - 1)[0] == E_INVALID
    # nothing selected is fine
    r = _raw(eng, [0, 0, 0, 0], [], 3, 100, 0)
    assert r[0] == 0 and r[1].tolist() == [0]
    # a resident step keeps no node_base_cov and may zero the arena: refused behind it, fine again behind the next stage call
    eng.profile_step(sset.avg_len())
    with pytest.raises(PantaxHipError) as e:
        eng.strain_segments(*sel, 3, 100)
    assert e.value.code == E_STATE and "resident step" in str(e.value)
    eng.get_node_abundances(fetch=False)
    _check(eng.strain_segments(*sel, 3, 100), exp)


# ---- the file seam -----------------------------------------------------------------------------------------------------------

HEADER = ["species_taxid", "strain_taxid", "genome_ID", "class", "rank", "start", "end", "span", "in_class", "n_segments", "n_nodes", "bases", "depth", "fraction",
          "threshold", "predicted_coverage"]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    yield from seam_world(tmp_path_factory, "pantax_sg", 32, 4, 5, 2500, 30000, present_frac=0.4, single_strain_every=4, with_ids=True)


def _f(x):
    return np.float64(x)


def _peak_depth(F, pc):
    return 0 if F == 0 else min(max(2, math.ceil(F * pc)), 2 ** 31)


def _expected_rows(sset, db, wd, eng, min_span, bridge, F):
    """the report rebuilt from the stage call, the chain reference and the run's strain table"""
    table = _lines(wd / "strain_abundance.txt")[1:]
    names = [g.name for g in sset.species]
    genome_hap = {r[0]: r[0].split("_ASM")[0] for r in _lines(db / "genomes_info.txt")[1:]}
    picked = [[] for _ in names]                                             # per species: (haplotype, row of the table)
    for i, t in enumerate(table):
        s = names.index(t[0])
        picked[s].append((sset.species[s].hap_names.index(genome_hap[t[2]]), i))
    off = np.concatenate([[0], np.cumsum([len(pk) for pk in picked])]).astype(np.uint64)
    hp = np.array([h for pk in picked for h, _ in pk], dtype=np.uint32)
    pd = np.array([_peak_depth(F, float(table[i][3])) for pk in picked for _, i in pk], dtype=np.uint64)
    entry_of_row = {i: int(off[s]) + k for s, pk in enumerate(picked) for k, (_, i) in enumerate(pk)}
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    eng.get_node_abundances(fetch=False)
    seg_off, hap_len, n_runs, run_len, run_max, cls, step, n_steps, start, ln, bases = eng.strain_segments(off, hp, pd, min(min_span, bridge + 1))
    dash = ["-"]
    out, n_chains = [], 0
    for i, t in enumerate(table):
        e = entry_of_row[i]
        G, thr = int(hap_len[e]), (int(pd[e]) if pd[e] else "-")
        out.append(t[:3] + ["strain", "-", 0, G, G] + dash * 6 + [thr, _f(t[3])])
        for k, name in enumerate(("gap_total", "peak_total")):
            out.append(t[:3] + [name] + dash * 3 + [int(run_max[e, k]), int(run_len[e, k]), int(n_runs[e, k])] + dash * 3 +
                       [_f(int(run_len[e, k])) / _f(G) if G else "-", thr if k else "-", _f(t[3])])
        lo, hi = int(seg_off[e]), int(seg_off[e + 1])
        rank = {GAP: 0, PEAK: 0}
        for c in chain(cls[lo:hi], start[lo:hi], ln[lo:hi], n_steps[lo:hi], bases[lo:hi], bridge, min_span):
            rank[c["class"]] += 1
            peak = c["class"] == PEAK
            out.append(t[:3] + ["peak" if peak else "gap", rank[c["class"]], c["start"], c["end"], c["span"], c["in_class"], c["n_segments"], c["n_steps"], c["bases"],
                                _f(c["bases"]) / _f(c["in_class"]), _f(c["in_class"]) / _f(c["span"]), thr if peak else "-", _f(t[3])])
            n_chains += 1
    return out, n_chains


def _same_rows(body, exp):
    assert len(body) == len(exp)
    for row, e in zip(body, exp):
        assert len(row) == len(HEADER) == len(e)
        for got, want in zip(row, e):
            if isinstance(want, np.floating):
                assert got != "-" and np.float64(got) == want, (row, e)
            else:
                assert got == str(want), (row, e)


def test_profile_seam_strain_segments(world, capfd, monkeypatch):
    from pantax_amd import _ffi
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng = world
    plain = root / "wd_plain"
    _profile(eng, db, plain, gaf)
    wd = root / "wd_sg"
    _profile(eng, db, wd, gaf, strain_segments_file=str(wd / "seg.tsv"))
    for f in ("species_abundance.txt", "strain_abundance.txt"):              # the option changes none of the tables
        assert open(wd / f, "rb").read() == open(plain / f, "rb").read()
    assert not os.path.exists(plain / "seg.tsv")
    rows = _lines(wd / "seg.tsv")
    assert rows[0] == HEADER
    exp, n_chains = _expected_rows(sset, db, wd, eng, 1000, 100, 10)         # the defaults
    _same_rows(rows[1:], exp)
    assert [r[3] for r in rows[1:4]] == ["strain", "gap_total", "peak_total"] and len(rows) - 1 == 3 * len(_lines(wd / "strain_abundance.txt")[1:]) + n_chains
    assert any(r[3] == "gap_total" and int(r[9]) > 0 for r in rows[1:]) and all(r[14] != "-" for r in rows[1:] if r[3] == "peak_total")
    full = open(wd / "seg.tsv", "rb").read()
    # other parameters: short spans, an explicit bridge of 0, a low factor -- chains of both classes; and peaks off
    w2 = root / "wd_sg_small"
    _profile(eng, db, w2, gaf, strain_segments_file=str(w2 / "seg.tsv"), strain_segments_min=40, strain_segments_bridge=0, strain_segments_peak=1)
    body2 = _lines(w2 / "seg.tsv")[1:]
    exp2, n2 = _expected_rows(sset, db, w2, eng, 40, 0, 1)
    _same_rows(body2, exp2)
    assert {"gap", "peak"} <= {r[3] for r in body2} and all(r[9] == "1" for r in body2 if r[3] in ("gap", "peak")) and n2 > n_chains
    w3 = root / "wd_sg_bridge"
    _profile(eng, db, w3, gaf, strain_segments_file=str(w3 / "seg.tsv"), strain_segments_min=40, strain_segments_bridge=300, strain_segments_peak="off")
    body3 = _lines(w3 / "seg.tsv")[1:]
    exp3, _ = _expected_rows(sset, db, w3, eng, 40, 300, 0)
    _same_rows(body3, exp3)
    assert not any(r[3] == "peak" for r in body3) and any(r[3] == "gap" and int(r[9]) > 1 for r in body3) and all(r[14] == "-" for r in body3)
    # beside the coverage track, whose selection it shares: neither file changes
    wb = root / "wd_sg_both"
    _profile(eng, db, wb, gaf, strain_segments_file=str(wb / "seg.tsv"), strain_coverage_file=str(wb / "cov.tsv"))
    wo = root / "wd_sg_cov"
    _profile(eng, db, wo, gaf, strain_coverage_file=str(wo / "cov.tsv"))
    assert open(wb / "seg.tsv", "rb").read() == full and open(wb / "cov.tsv", "rb").read() == open(wo / "cov.tsv", "rb").read()
    # a species-only run writes nothing and says so; the strain-only resume behind it writes the same file
    wr = root / "wd_sg_resume"
    capfd.readouterr()
    _profile(eng, db, wr, gaf, species=True, strain=False, out_binning_file=str(wr / "reads_classification.tsv"), strain_segments_file=str(wr / "seg_species_only.tsv"))
    assert not os.path.exists(wr / "seg_species_only.tsv") and "no strain step" in capfd.readouterr().err
    _profile(eng, db, wr, gaf, species=False, strain=True, strain_segments_file=str(wr / "seg.tsv"))
    assert open(wr / "seg.tsv", "rb").read() == full
    # the command-line front end: the defaults, and the three parameters
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_sg_cli"
    wc.mkdir()
    base = [exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0"]
    r = subprocess.run(base + ["--strain-segments", str(wc / "seg.tsv")], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc / "seg.tsv", "rb").read() == full
    wc2 = root / "wd_sg_cli2"                                                # (a second run into the same work directory would resume, with the strain step done)
    wc2.mkdir()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wc2), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0", "--strain-segments",
                        str(wc2 / "seg.tsv"), "--strain-segments-min", "40", "--strain-segments-bridge", "0", "--strain-segments-peak", "1"],
                       cwd=str(wc2), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc2 / "seg.tsv", "rb").read() == open(w2 / "seg.tsv", "rb").read()
    r = subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=120)
    assert "--strain-segments-bridge" in r.stdout + r.stderr and "--strain-segments-peak F|off" in r.stdout + r.stderr
    # several ranks: refused on every rank with the table's wording, before any collective
    for rank in range(2):
        wn = root / ("wd_sg_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, strain_segments_file=str(wn / "seg.tsv"))
        assert e.value.code == E_INVALID and "the segment report (strain_segments_file) needs one rank and an unsharded ingest (world_size 2)" in str(e.value)
        assert not os.path.exists(wn / "seg.tsv")
    # a caller compiled against the header before these fields: its struct ends behind strain_em_iterations, the report reads as off
    real = _ffi.ProfileExt

    class OldExt(real):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.struct_size = 88

    monkeypatch.setattr(_ffi, "ProfileExt", OldExt)
    wold = root / "wd_sg_old"
    _profile(eng, db, wold, gaf, strain_fit_file=str(wold / "fit.tsv"), strain_segments_file=str(wold / "seg.tsv"))
    monkeypatch.setattr(_ffi, "ProfileExt", real)
    assert os.path.exists(wold / "fit.tsv") and not os.path.exists(wold / "seg.tsv")
    assert open(wold / "strain_abundance.txt", "rb").read() == open(wd / "strain_abundance.txt", "rb").read()
