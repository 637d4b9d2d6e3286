"""GPU tests of the per-read strain assignment (pantax_hip_read_strains, --read-strains).  The expected values come from the numpy
restatement of the contract below (include/pantax_hip.h): N(r) = the distinct nodes of the read's walk, C(r) = the
candidates whose walk visits all of them, the argmax of the weight over C(r) with ties to the smallest haplotype index, and the
posterior summed in ascending haplotype index -- the same order as the library, so posteriors compare bitwise."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile, seam_world

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


def _bin(sset_species, reads):
    from oracle import oracle as orc
    return orc.bin_reads(reads.step_off, reads.node_id, [g.range_start for g in sset_species], [g.range_end for g in sset_species])


def _expected(species, step_off, node_id, sp, counted, cand_off, cand_hap, cand_w, fill):
    """the contract, read by read: (hap, n, posterior) [R]; reads with sp < 0 keep `fill`"""
    hap, n, post = (np.array(a, copy=True) for a in fill)
    member = []
    for s, g in enumerate(species):
        ks = [(int(cand_hap[c]), float(cand_w[c])) for c in range(int(cand_off[s]), int(cand_off[s + 1]))]
        ks.sort()
        m = np.zeros((g.n_nodes, len(ks)), dtype=bool)
        for j, (h, _) in enumerate(ks):
            m[g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])].astype(np.int64), j] = True
        member.append((ks, m))
    for r in range(len(sp)):
        s = int(sp[r])
        if s < 0:
            continue
        ks, m = member[s]
        if not counted[r] or not ks:
            hap[r], n[r], post[r] = NONE, -1, 0.0
            continue
        nodes = np.unique(node_id[int(step_off[r]):int(step_off[r + 1])].astype(np.int64) - species[s].range_start)
        ok = np.nonzero(m[nodes].all(axis=0))[0]
        if len(ok) == 0:
            hap[r], n[r], post[r] = NONE, 0, 0.0
            continue
        best, besth, tot = -np.inf, None, 0.0
        for j in ok:                                   # ascending haplotype index
            h, w = ks[j]
            tot += w
            if w > best:
                best, besth = w, h
        hap[r], n[r], post[r] = besth, len(ok), best / tot
    return hap, n, post


def _check(got, exp):
    assert np.array_equal(got[0], exp[0])
    assert np.array_equal(got[1], exp[1])
    assert np.array_equal(got[2].view(np.uint64), exp[2].view(np.uint64))


def _cands(species, rng, pick):
    """pick(s, H) -> list of haplotypes; weights drawn with a few ties"""
    off, hp, w = [0], [], []
    for s, g in enumerate(species):
        hs = list(pick(s, g.n_paths))
        rng.shuffle(hs)                                 # any order on the way in
        ws = rng.choice([1.0, 2.5, 7.25], size=len(hs)) if s % 2 else rng.random(len(hs)) * 10 + 0.1
        hp += hs
        w += list(ws)
        off.append(len(hp))
    return np.array(off, dtype=np.uint64), np.array(hp, dtype=np.uint32), np.array(w, dtype=np.float64)


def _run(eng, species, reads, flags, cands, fill=None):
    eng.upload_db(species)
    eng.upload_reads(reads.step_off, reads.node_id, reads.pstart, reads.pend, reads.qlen, reads.mapq, flags)
    eng.rcls_profile(want_species=False)
    R = reads.n_reads
    if fill is None:
        fill = (np.full(R, 12345, dtype=np.uint32), np.full(R, -7, dtype=np.int32), np.full(R, 0.5))
    got = eng.read_strains(*cands, fill=fill)
    sp = _bin(species, reads)
    counted = np.ones(R, dtype=bool) if flags is None else np.asarray(flags) == 0
    exp = _expected(species, reads.step_off, reads.node_id, sp, counted, *cands, fill)
    return got, exp, sp


def _with_long_walks(sset, rng, n_extra, steps):
    """append reads whose walk is a stretch of `steps` consecutive path steps of a haplotype (walks of > 64 and > 4096 steps)"""
    import synthdata as synth
    rd = sset.reads
    nodes, ks = [], []
    for _ in range(n_extra):
        g = sset.species[int(rng.integers(0, len(sset.species)))]
        h = int(rng.integers(0, g.n_paths))
        b, e = int(g.path_off[h]), int(g.path_off[h + 1])
        k = min(steps, e - b)
        i0 = b + int(rng.integers(0, e - b - k + 1))
        nodes.append(g.path_nodes[i0:i0 + k].astype(np.uint32) + np.uint32(g.range_start))
        ks.append(k)
    step_off = np.concatenate([rd.step_off, rd.step_off[-1] + np.cumsum(np.array(ks, dtype=np.uint64))])
    one = lambda v: np.full(n_extra, v, dtype=np.int64)
    return synth.PackedReads(step_off, np.concatenate([rd.node_id] + nodes), None, np.concatenate([rd.pstart, one(0)]),
                             np.concatenate([rd.pend, one(1)]), np.concatenate([rd.qlen, one(30000)]), np.concatenate([rd.mapq, one(60)]),
                             np.concatenate([rd.plen, one(30000)]))


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def test_read_strains_narrow_species(eng, set_opt):
    """species of <= 64 haplotypes (node -> haplotype words): all haplotypes, a subset, none; short reads; route walk bitwise equal"""
    import synthdata as synth
    sset = synth.make_set(901, 3, 6, 20000, 30000, present_frac=0.6)
    rng = np.random.default_rng(1)
    cands = _cands(sset.species, rng, lambda s, H: range(H) if s == 0 else ([] if s == 2 else [0, 2, 3]))
    got, exp, sp = _run(eng, sset.species, sset.reads, None, cands)
    _check(got, exp)
    assert (exp[1] > 1).sum() > 100 and (exp[1] == 0).sum() > 0 and (exp[1] == -1).sum() > 0   # shared reads, nothing compatible, no candidates
    assert (sp < 0).sum() > 0 and np.all(got[1][sp < 0] == -7)                                 # "U": the caller's values
    set_opt(eng, "read_strain_route", "walk")
    got2 = eng.read_strains(*cands, fill=(np.full(sset.reads.n_reads, 12345, dtype=np.uint32), np.full(sset.reads.n_reads, -7, dtype=np.int32),
                                          np.full(sset.reads.n_reads, 0.5)))
    _check(got2, got)


@pytest.mark.parametrize("H", [100, 200])
def test_read_strains_wide_species(eng, set_opt, H):
    """species of more than 64 haplotypes: compact multi-word masks from the candidates' walks (> 64 candidates, and all of them)"""
    import synthdata as synth
    sset = synth.make_set(902 + H, 2, H, 8000, 12000, present_frac=0.6)
    rng = np.random.default_rng(H)
    cands = _cands(sset.species, rng, lambda s, n: range(n) if s == 0 else sorted(rng.choice(n, size=n - 20, replace=False).tolist()))
    got, exp, _ = _run(eng, sset.species, sset.reads, None, cands)
    _check(got, exp)
    assert (exp[1] > 64).sum() > 0
    set_opt(eng, "read_strain_route", "walk")
    _check(eng.read_strains(*cands, fill=got), got)


def test_read_strains_long_walks(eng, set_opt):
    """long reads: walks of > 64 steps and of > 4096 steps (per-group partials combined across groups), narrow and wide species"""
    import synthdata as synth
    rng = np.random.default_rng(3)
    for H, n in ((6, 400), (90, 150)):
        sset = synth.make_set(903 + H, 2, H, n, 300000, long_reads=True, present_frac=0.6)
        reads = _with_long_walks(sset, rng, 12, 5000)
        k = np.diff(reads.step_off.astype(np.int64))
        assert (k > 64).sum() > n // 2 and (k > 4096).sum() >= 6
        cands = _cands(sset.species, rng, lambda s, m: range(m) if s == 0 else list(range(0, m, 2)))
        got, exp, _ = _run(eng, sset.species, reads, None, cands)
        _check(got, exp)
        assert (exp[1] >= 1).sum() > 0
        set_opt(eng, "read_strain_route", "walk")
        _check(eng.read_strains(*cands, fill=got), got)
        set_opt(eng, "read_strain_route", None)


def test_read_strains_sentinels_and_state(eng):
    """a db of SOME of the species: the other reads keep the caller's values; dropped reads (flags) are "not counted"; reads not binned
    against the db are refused"""
    import synthdata as synth
    from pantax_amd._ffi import PantaxHipError
    sset = synth.make_set(904, 3, 5, 6000, 20000, present_frac=0.6)
    rng = np.random.default_rng(4)
    R = sset.reads.n_reads
    flags = np.zeros(R, dtype=np.uint8)
    flags[rng.choice(R, size=300, replace=False)] = rng.choice([1, 2], size=300).astype(np.uint8)   # null field / duplicate-id rule
    part = [sset.species[1]]
    cands = _cands(part, rng, lambda s, H: range(H))
    got, exp, sp = _run(eng, part, sset.reads, flags, cands)
    _check(got, exp)
    assert np.all(got[1][(sp == 0) & (flags != 0)] == -1) and ((sp == 0) & (flags != 0)).sum() > 10
    assert np.all(got[1][sp < 0] == -7) and (sp < 0).sum() > R // 10
    eng.upload_db(sset.species)                          # the reads were binned against the previous db
    with pytest.raises(PantaxHipError) as e:
        eng.read_strains(*_cands(sset.species, rng, lambda s, H: [0]))
    assert e.value.code == -7


# ---- the file seam -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world(tmp_path_factory):
    yield from seam_world(tmp_path_factory, "pantax_rs", 31, 4, 5, 30000, 30000, present_frac=0.4, single_strain_every=4, with_ids=True)


def _tables(wd):
    return [open(wd / f, "rb").read() for f in ("species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt")]


def test_profile_seam_read_strains(world):
    sset, root, db, gaf, eng = world
    _profile(eng, db, root / "wd_plain", gaf)
    wd = root / "wd_rs"
    _profile(eng, db, wd, gaf, out_binning_file=str(wd / "reads_classification.tsv"), read_strain_file=str(wd / "read_strains.tsv"))
    assert _tables(wd) == _tables(root / "wd_plain")     # the option changes none of the tables
    rep, rs = _lines(wd / "reads_classification.tsv"), _lines(wd / "read_strains.tsv")
    assert len(rs) == len(rep) == sset.reads.n_reads
    assert [r[0] for r in rs] == [r[0] for r in rep] and [r[1] for r in rs] == [r[2] for r in rep]
    # the restatement, from the tables: candidates = the rows of strain_abundance.txt, weight = their predicted_coverage (full = 1)
    gi = _lines(db / "genomes_info.txt")[1:]
    genome_hap = {r[0]: r[0].split("_ASM")[0] for r in gi}
    hap_meta = {}
    for r in gi:
        hap_meta.setdefault(r[0].split("_ASM")[0], (r[0], r[1]))
    names = [g.name for g in sset.species]
    cand = {s: [] for s in range(len(names))}
    for r in _lines(wd / "strain_abundance.txt")[1:]:
        s = names.index(r[0])
        cand[s].append((sset.species[s].hap_names.index(genome_hap[r[2]]), float(r[3])))
    off = np.cumsum([0] + [len(cand[s]) for s in range(len(names))]).astype(np.uint64)
    ch = np.array([h for s in range(len(names)) for h, _ in cand[s]], dtype=np.uint32)
    cw = np.array([w for s in range(len(names)) for _, w in cand[s]], dtype=np.float64)
    R = sset.reads.n_reads
    sp = np.array([names.index(r[2]) if r[2] != "U" else -1 for r in rep])
    sp_sel = np.where(np.isin(sp, [s for s in cand if cand[s]]), sp, -1)   # species without rows (or not selected): "not counted"
    exp = _expected(sset.species, sset.reads.step_off, sset.reads.node_id, sp_sel, np.ones(R, dtype=bool), off, ch, cw,
                    (np.full(R, NONE, dtype=np.uint32), np.full(R, -1, dtype=np.int32), np.zeros(R)))
    assert (exp[1] > 0).sum() > R // 4
    for r in range(R):
        row = rs[r][2:]
        if exp[1][r] < 0:
            assert row == ["U", "U", "-", "0"], (r, rs[r])
        elif exp[1][r] == 0:
            assert row == ["U", "U", "0", "0"], (r, rs[r])
        else:
            s = sp_sel[r]
            gid, staxid = hap_meta[sset.species[s].hap_names[exp[0][r]]]
            assert row[:3] == [gid, staxid, str(exp[1][r])], (r, rs[r])
            assert float(row[3]) == exp[2][r], (r, rs[r])


@pytest.mark.parametrize("image_cache", [0, 1])
def test_profile_seam_read_strains_in_groups(world, set_opt, image_cache):
    sset, root, db, gaf, eng = world
    if image_cache:
        db2 = root / "db_rs_img"
        if not db2.exists():
            shutil.copytree(db, db2)
            _profile(eng, db2, root / "wd_rs_img_prime", gaf, image_cache=2)
        db = db2
    steps = sorted(int(g.path_off[-1]) for g in sset.species)
    outs = {}
    for name, limit in [("one", None), ("each", 1), ("pairs", steps[-1] + steps[-2])]:
        wd = root / ("wd_rs_groups_%s_%d" % (name, image_cache))
        set_opt(eng, "db_path_steps_max", limit)
        try:
            _profile(eng, db, wd, gaf, image_cache=image_cache, read_strain_file=str(wd / "rs.tsv"))
        finally:
            set_opt(eng, "db_path_steps_max", None)
        outs[name] = open(wd / "rs.tsv", "rb").read()
    assert outs["one"].count(b"\n") == sset.reads.n_reads
    assert outs["each"] == outs["one"] and outs["pairs"] == outs["one"]


def test_profile_seam_read_strains_resume_cli_and_refusals(world, capfd):
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng = world
    wd = root / "wd_rs_full"
    _profile(eng, db, wd, gaf, read_strain_file=str(wd / "rs.tsv"))
    full = open(wd / "rs.tsv", "rb").read()
    # the strain-only resume from reads_classification.tsv writes the same file
    wr = root / "wd_rs_resume"
    _profile(eng, db, wr, gaf, species=True, strain=False, out_binning_file=str(wr / "reads_classification.tsv"),
             read_strain_file=str(wr / "rs_species_only.tsv"))
    assert not os.path.exists(wr / "rs_species_only.tsv")
    _profile(eng, db, wr, gaf, species=False, strain=True, read_strain_file=str(wr / "rs.tsv"))
    assert open(wr / "rs.tsv", "rb").read() == full
    # no strain step (the table exists, no --force): nothing written, a note on stderr
    capfd.readouterr()
    _profile(eng, db, wr, gaf, species=True, strain=True, read_strain_file=str(wr / "rs_again.tsv"))
    assert not os.path.exists(wr / "rs_again.tsv") and "no strain step" in capfd.readouterr().err
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_rs_cli"
    wc.mkdir()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0",
                        "--read-strains", str(wc / "rs.tsv")], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc / "rs.tsv", "rb").read() == full
    # several ranks: refused on every rank, before any collective
    for rank in range(2):
        wn = root / ("wd_rs_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, read_strain_file=str(wn / "rs.tsv"))
        assert e.value.code == -1
        assert not os.path.exists(wn / "rs.tsv")
