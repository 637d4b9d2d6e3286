"""GPU test of the pipeline seam (pantax_hip_profile == profile::profile, profile.rs:3325): a small
synthetic DB + GAF on disk -> species_abundance.txt / strain_abundance.txt, checked against the
oracle run on the same inputs (numeric comparison; polars' float text is not byte-pinned)."""
import os

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import select_reads

pytestmark = pytest.mark.gpu


def _read_tsv(path):
    with open(path) as f:
        hdr = f.readline().rstrip("\n").split("\t")
        return hdr, [line.rstrip("\n").split("\t") for line in f]


def _oracle_tables(sset, fr=0.3, fc=0.46, sr=0.85, sd=0.2, min_ab=1e-4, strain_drop=None, min_cov=0, shift=False, min_depth=0, ds=None,
                   mode=2, sample_nodes=0, solver_semantics=0):
    from oracle import oracle as orc
    rd = sset.reads
    S = len(sset.species)
    sp = orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in sset.species], [g.range_end for g in sset.species])
    counts = orc.species_counts(sp, rd.qlen, rd.mapq, S)
    keep, absolute, abundance = orc.species_profile(sp, rd.qlen, counts, sset.avg_len())
    species_rows = sorted([(sset.species[s].name, abundance[s], absolute[s]) for s in range(S) if keep[s]], key=lambda r: -r[1])
    rows = []
    for s, g in enumerate(sset.species):
        if not keep[s] or not abundance[s] > min_ab:
            continue
        is_pan = 1 if g.n_paths > 1 else 0            # species_range.txt column 4 (load_species_range, profile.rs:553-656)
        if (mode == 0 and is_pan != 0) or (mode == 1 and is_pan != 1) or (ds is not None and g.name not in ds):
            continue
        G = orc.Graph(g.node_len, g.path_off, g.path_nodes)
        T = orc.TrioTable(G)
        mine = sp == s if strain_drop is None else (sp == s) & ~strain_drop
        so, nid, ps, pe = select_reads(rd, np.nonzero(mine)[0])
        b, c, tb, _ = orc.node_coverage(G, T, g.range_start, so, nid, ps, pe)
        rc, met, nc, o1, o2 = orc.optimize_species(G, T, b, c, tb, fr=fr, fc=fc, sr=sr, shift=shift, min_depth=min_depth, sample_nodes=sample_nodes,
                                                   solver_semantics=solver_semantics)
        assert rc == 0
        orc.abundance_constraint(absolute[s], met)
        d = orc.metrics_to_dicts(met)
        for h, m in enumerate(d):
            cov = m["predicted_coverage"]
            if cov is None:
                continue
            if (len(d) > 1 or (m["total_cov_diff"] is not None and m["total_cov_diff"] <= sd)) and cov >= min_cov and cov != 0.0:
                rows.append((g.name, g.hap_names[h], m))
    tot = sum(r[2]["predicted_coverage"] for r in rows)
    out = [(sp_, hap, m["predicted_coverage"], m["predicted_coverage"] / tot, m) for sp_, hap, m in rows]
    out.sort(key=lambda r: -r[3])
    return species_rows, out, sp


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import synthdata as synth
    from pantax_amd.engine import Engine
    sset = synth.make_set(31, 4, 5, 30000, 30000, present_frac=0.4, single_strain_every=4, with_ids=False)
    root = tmp_path_factory.mktemp("pantax")
    db = root / "db"
    db.mkdir()
    synth.write_db(sset, str(db))
    gaf = root / "gfa_mapped.gaf"
    synth.write_gaf(sset.reads, str(gaf))
    eng = Engine(0)
    yield sset, root, db, gaf, eng
    eng.close()


def _check_outputs(wd, sset, exp_species, exp_strain, rounded=False):
    hdr, rows = _read_tsv(os.path.join(wd, "species_abundance.txt"))
    assert hdr == ["species_taxid", "predicted_abundance", "predicted_coverage"]
    assert [r[0] for r in rows] == [r[0] for r in exp_species]
    for r, e in zip(rows, exp_species):
        assert float(r[1]) == pytest.approx(e[1], rel=1e-12) and float(r[2]) == pytest.approx(e[2], rel=1e-12)
    hdr, rows = _read_tsv(os.path.join(wd, "strain_abundance.txt"))
    assert hdr == ["species_taxid", "strain_taxid", "genome_ID", "predicted_coverage", "predicted_abundance", "path_base_cov",
                   "unique_trio_fraction", "uniq_trio_cov_mean", "first_sol", "strain_cov_diff", "total_cov_diff"]
    assert len(rows) == len(exp_strain) and len(rows) > 0
    for r, (sp_, hap, cov, ab, m) in zip(rows, exp_strain):
        assert r[0] == sp_ and r[2].startswith(hap)
        assert float(r[4]) == pytest.approx(ab, rel=1e-7)
        if rounded:   # full = false: every metric column but predicted_abundance goes through .round(2) (profile.rs:3266-3284)
            assert abs(float(r[3]) - cov) <= 0.005 + 1e-9 and len(r[3].partition(".")[2]) <= 2
        else:
            assert float(r[3]) == pytest.approx(cov, rel=1e-7)
        for col, key in [(5, "path_base_cov"), (6, "unique_trio_fraction"), (7, "uniq_trio_cov_mean"), (8, "first_sol"),
                         (9, "strain_cov_diff"), (10, "total_cov_diff")]:
            if m[key] is None:
                assert r[col] == ""
            elif rounded:
                assert abs(float(r[col]) - m[key]) <= 0.005 + 1e-9 and len(r[col].partition(".")[2]) <= 2, (key, r)
            else:
                assert float(r[col]) == pytest.approx(m[key], rel=1e-7, abs=1e-9), (key, r)
    assert abs(sum(float(r[4]) for r in rows) - 1.0) < 1e-9


def test_profile_seam_bin_and_gfa(world):
    sset, root, db, gaf, eng = world
    exp_species, exp_strain, sp = _oracle_tables(sset)
    cwd = os.getcwd()
    # the same graphs behind the two stream codecs of zip.rs:191-223 (pyarrow writes those container formats)
    import pyarrow as pa
    for f in os.listdir(db / "species_graph_info"):
        if f.endswith(".bin"):
            raw = open(db / "species_graph_info" / f, "rb").read()
            (db / "species_graph_info" / (f + ".lz4")).write_bytes(pa.Codec("lz4").compress(raw, asbytes=True))
            (db / "species_graph_info" / (f + ".zst")).write_bytes(pa.Codec("zstd").compress(raw, asbytes=True))
    for name, zip_ in [("wd_bin", "serialize"), ("wd_gfa", None), ("wd_lz", "lz"), ("wd_zstd", "zstd")]:
        wd = root / name
        wd.mkdir()
        os.chdir(str(wd))   # ori_strain_abundance.txt goes to the current directory (profile.rs:3217)
        try:
            eng.profile(str(db), str(wd), str(gaf), zip=zip_, out_binning_file=str(wd / "reads_classification.tsv"))
        finally:
            os.chdir(cwd)
        _check_outputs(str(wd), sset, exp_species, exp_strain)
        assert os.path.exists(wd / "ori_strain_abundance.txt")
        # binning report: read_id, mapq, species, read_len without header, one row per GAF line
        with open(wd / "reads_classification.tsv") as f:
            rep = [l.rstrip("\n").split("\t") for l in f]
        assert len(rep) == sset.reads.n_reads
        names = [g.name for g in sset.species]
        assert [r[2] for r in rep[:200]] == [names[i] if i >= 0 else "U" for i in sp[:200]]


@pytest.mark.parametrize("zip_,image_cache", [("serialize", 0), (None, 0), ("serialize", 1)])
def test_profile_seam_in_groups_of_species_writes_the_same_files(world, zip_, image_cache, set_opt):
    """A selection of more path steps than one resident db addresses (2^32: BASELINE configs[4] on one GPU) goes through the device in groups of
    species, one after the other, inside ONE pantax_hip_profile call (species are independent from a4 on, profile.rs:3297-3319).  Forced here by a
    tiny limit (option db_path_steps_max: every species a group of its own, then two per group): the tables are the same BYTES as the one-db
    run's -- from bincode files, GFA text and device-ready images."""
    sset, root, db, gaf, eng = world
    cwd = os.getcwd()
    outs = {}
    steps = sorted(int(g.path_off[-1]) for g in sset.species)
    if image_cache:   # leave images behind first -- in a copy of the db: the module's db directory stays free of images for the other tests
        import shutil
        db = root / "db_groups_img"
        shutil.copytree(world[2], db)
        wd0 = root / ("wd_groups_img_prime_%s" % zip_)
        wd0.mkdir()
        os.chdir(str(wd0))
        try:
            eng.profile(str(db), str(wd0), str(gaf), zip=zip_, image_cache=2)
        finally:
            os.chdir(cwd)
    for name, limit in [("one", None), ("each", 1), ("pairs", steps[-1] + steps[-2])]:
        wd = root / ("wd_groups_%s_%s_%d" % (name, zip_, image_cache))
        wd.mkdir()
        set_opt(eng, "db_path_steps_max", limit)
        os.chdir(str(wd))
        try:
            eng.profile(str(db), str(wd), str(gaf), zip=zip_, image_cache=image_cache)
        finally:
            os.chdir(cwd)
            set_opt(eng, "db_path_steps_max", None)
        outs[name] = [open(wd / f, "rb").read() for f in ("species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt")]
    assert len(outs["one"][1].splitlines()) > 2
    assert outs["each"] == outs["one"] and outs["pairs"] == outs["one"]


def test_profile_seam_resume_strain_only(world):
    """--strain after an earlier --species run (profile.rs:3365-3417): same strain table."""
    sset, root, db, gaf, eng = world
    exp_species, exp_strain, sp = _oracle_tables(sset)
    wd = root / "wd_resume"
    wd.mkdir()
    cwd = os.getcwd()
    os.chdir(str(wd))
    try:
        eng.profile(str(db), str(wd), str(gaf), species=True, strain=False, out_binning_file=str(wd / "reads_classification.tsv"))
        assert os.path.exists(wd / "species_abundance.txt") and not os.path.exists(wd / "strain_abundance.txt")
        eng.profile(str(db), str(wd), str(gaf), species=False, strain=True)
        # existing outputs short-circuit the run unless --force (profile.rs:136-156)
        before = os.path.getmtime(wd / "strain_abundance.txt")
        eng.profile(str(db), str(wd), str(gaf), species=True, strain=True)
        assert os.path.getmtime(wd / "strain_abundance.txt") == before
    finally:
        os.chdir(cwd)
    _check_outputs(str(wd), sset, exp_species, exp_strain)


def test_profile_seam_duplicate_read_ids(world):
    """Read ids that repeat (GraphAligner reports several alignments of a long read): an id whose alignments all bin to
    one species keeps them all, an id seen in two species loses them all at the strain level, and the species table
    still counts every row (profile.rs:361-463)."""
    import copy
    import synthdata as synth
    sset, root, db, gaf, eng = world
    rd = copy.copy(sset.reads)
    R = rd.n_reads
    _, _, sp = _oracle_tables(sset)
    ids = ["S0R%d/1" % r for r in range(R)]
    rng = np.random.default_rng(5)
    mapped = np.nonzero(sp >= 0)[0]
    drop = np.zeros(R, bool)
    n_same = n_mixed = 0
    for a, b in rng.choice(mapped, size=(3000, 2), replace=False):
        ids[b] = ids[a]
        if sp[a] == sp[b]:
            n_same += 1
        else:
            drop[a] = drop[b] = True
            n_mixed += 1
    assert n_same > 50 and n_mixed > 50
    rd.read_id = ids
    gaf2 = root / "dup.gaf"
    synth.write_gaf(rd, str(gaf2))
    exp_species, exp_strain, _ = _oracle_tables(sset, strain_drop=drop)
    wd = root / "wd_dup"
    wd.mkdir()
    cwd = os.getcwd()
    os.chdir(str(wd))
    try:
        eng.profile(str(db), str(wd), str(gaf2))
    finally:
        os.chdir(cwd)
    _check_outputs(str(wd), sset, exp_species, exp_strain)
    # and the rule changes the answer here: without it the strain table differs
    _, plain, _ = _oracle_tables(sset)
    assert any(abs(a[2] - b[2]) > 1e-9 for a, b in zip(plain, exp_strain)) or len(plain) != len(exp_strain)


def _piece_size_that_overflows_the_id_set(text):
    """A gaf_piece_bytes (64 KiB .. a quarter of the text) under which the device tokenizer's id hash set is too small for `text`, or None.  Replays the
    rule of tokenize_piece (stage_gaf.hip): the first piece's rows R0 size the joined per-read columns, max(R0, int(R0 * 1.03 * size / piece size) + 1024);
    the set gets the first power of two (from 1024) that is at least twice that; it is given up once the reads so far exceed 0.7 of its slots.
    This only CHOOSES AN INPUT: which route the tokenizer took is asserted on its own counters."""
    size = len(text)
    is_row = lambda l: bool(l.rstrip(b"\r")) and not l.startswith(b"@")
    n_rows = sum(1 for l in text.split(b"\n") if is_row(l))
    piece = 65536
    while piece <= size // 4:
        k = text.rfind(b"\n", 0, piece)
        if k < 0:
            return None
        first = text[:k + 1]
        r0 = sum(1 for l in first.split(b"\n") if is_row(l))
        cap_r = max(r0, min(0xFFFFFFFE, int(r0 * (1.03 * size / len(first))) + 1024))
        slots = 1024
        while slots < 2 * cap_r:
            slots <<= 1
        if n_rows > 0.7 * slots:
            return piece
        piece *= 2
    return None


def test_profile_seam_duplicate_read_ids_decided_by_the_hash_sort(world, set_opt):
    """test_profile_seam_duplicate_read_ids with the duplicates found on the tokenizer's OTHER route: a block of comment lines behind the first 20 reads
    makes the first piece sparse, the id hash set sized from it overflows, and the verdict "some reads share an id" comes from the sort of all id hashes
    and dup_count_kernel.  A false "all distinct" there would skip the duplicate-id rule (profile.rs:361-437) and give the plain strain table."""
    import copy
    import synthdata as synth
    from pantax_amd import io as pio
    sset, root, db, gaf, eng = world
    rd = copy.copy(sset.reads)
    R = rd.n_reads
    _, _, sp = _oracle_tables(sset)
    ids = ["S0R%d/1" % r for r in range(R)]
    rng = np.random.default_rng(5)
    mapped = np.nonzero(sp >= 0)[0]
    drop = np.zeros(R, bool)
    n_same = n_mixed = 0
    for a, b in rng.choice(mapped, size=(3000, 2), replace=False):
        ids[b] = ids[a]
        if sp[a] == sp[b]:
            n_same += 1
        else:
            drop[a] = drop[b] = True
            n_mixed += 1
    assert n_same > 50 and n_mixed > 50
    rd.read_id = ids
    gaf2 = root / "dup_sparse_head.gaf"
    synth.write_gaf(rd, str(gaf2))
    lines = gaf2.read_bytes().split(b"\n")
    text = b"\n".join(lines[:20]) + b"\n" + (b"@" + b"x" * 98 + b"\n") * 3000 + b"\n".join(lines[20:])
    gaf2.write_bytes(text)
    piece = _piece_size_that_overflows_the_id_set(text)
    if piece is None:
        pytest.skip("no piece size between 64 KiB and a quarter of the file overflows the id hash set of this text")
    set_opt(eng, "gaf_piece_bytes", str(piece))
    # the same text through the same tokenizer, where its route can be read: the sort decided, and found duplicates
    view = pio.load_gaf(gaf2, engine=eng, ids=True)
    assert view["id_check"] == 2 and view["n_pieces"] > 1, {k: view[k] for k in ("id_check", "ids_distinct", "n_pieces")}
    exp_species, exp_strain, _ = _oracle_tables(sset, strain_drop=drop)
    wd = root / "wd_dup_sort"
    wd.mkdir()
    cwd = os.getcwd()
    os.chdir(str(wd))
    try:
        eng.profile(str(db), str(wd), str(gaf2))
    finally:
        os.chdir(cwd)
    _check_outputs(str(wd), sset, exp_species, exp_strain)
    assert view["ids_distinct"] == 0
    # and the rule changes the answer here: without it the strain table differs
    _, plain, _ = _oracle_tables(sset)
    assert any(abs(a[2] - b[2]) > 1e-9 for a, b in zip(plain, exp_strain)) or len(plain) != len(exp_strain)


def test_profile_seam_default_sample_limit(world):
    """--sample 500000 (the reference's default, cli.rs:227) leaves species with fewer valid rows alone."""
    sset, root, db, gaf, eng = world
    exp_species, exp_strain, sp = _oracle_tables(sset)
    wd = root / "wd_sample"
    wd.mkdir()
    cwd = os.getcwd()
    os.chdir(str(wd))
    try:
        eng.profile(str(db), str(wd), str(gaf), sample_nodes=500000)
    finally:
        os.chdir(cwd)
    _check_outputs(str(wd), sset, exp_species, exp_strain)


@pytest.mark.parametrize("name,kw,okw,rounded", [
    ("ds", dict(designated_species="1001, 1003"), dict(ds=["1001", "1003"]), False),              # --ds: only these species reach the strain level
    ("mode0", dict(mode=0), dict(mode=0), False),                                                 # species with a single genome only (is_pan = 0)
    ("mode1", dict(mode=1), dict(mode=1), False),                                                 # pan species only
    ("cut", dict(min_species_abundance=0.2), dict(min_ab=0.2), False),                            # -a: species below the cut are not profiled
    ("mincov", dict(min_cov=4, sd=0.05), dict(min_cov=4, sd=0.05), False),                        # --min_cov / --sd of abundance_est
    ("shift", dict(shift=True, fr=0.5, min_depth=1), dict(shift=True, fr=0.5, min_depth=1), False),
    ("round", dict(full=False), dict(), True),                                                    # two-decimal table
    # --sample_test (cli.rs:230-232): 500 rows of sample_sorted whatever --sample says (profile.rs:1387-1393, :2738-2744)
    ("sample_test", dict(sample_test=True, sample_nodes=500000), dict(sample_nodes=500), False),
    # --solver highs: the second solve's solution through highs_opt's slice (profile.rs:2865-2879); a tight --fc makes candidates fall in the second filter
    ("highs", dict(solver_semantics=1, fc=0.05, sr=0.99), dict(solver_semantics=1, fc=0.05, sr=0.99), False),
])
def test_profile_seam_options(world, name, kw, okw, rounded):
    """The option branches of load_species_range / optimize_otu / abundance_est through the file seam (profile.rs:553-656,
    :2884-3026, :3091-3289) against the oracle with the same options."""
    sset, root, db, gaf, eng = world
    exp_species, exp_strain, _ = _oracle_tables(sset, **okw)
    if name != "round":
        assert exp_strain != _oracle_tables(sset)[1]          # the option changes the answer on this data
    if name == "highs":                                       # ... and so does the slice itself: Gurobi's reading of the same options gives other rows
        assert exp_strain != _oracle_tables(sset, fc=0.05, sr=0.99)[1]
    wd = root / ("wd_opt_" + name)
    wd.mkdir()
    cwd = os.getcwd()
    os.chdir(str(wd))
    try:
        eng.profile(str(db), str(wd), str(gaf), **kw)
    finally:
        os.chdir(cwd)
    _check_outputs(str(wd), sset, exp_species, exp_strain, rounded=rounded)


def test_profile_seam_errors(world):
    from pantax_amd.engine import PantaxHipError
    sset, root, db, gaf, eng = world
    wd = root / "wd_err"
    wd.mkdir()
    with pytest.raises(PantaxHipError):
        eng.profile(str(db), str(wd), str(root / "missing.gaf"))
    with pytest.raises(PantaxHipError):
        eng.profile(str(db), str(wd), str(gaf), sample_nodes=-1)
    with pytest.raises(PantaxHipError):
        eng.profile(str(db), str(wd), str(gaf), species=False, strain=False)


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("piece", [None, "300000"])
def test_resident_gaf_load_equals_the_gaf_reader_oracle(eng, tmp_path, piece, set_opt):
    """pantax_hip_reads_load_gaf: the resident reads are the reads of the text -- the host columns, the species per read and the
    coverage integers of the packed upload of what oracle/gaf_reader.py (a reading of load_gaf_file_lazy, rcls.rs:119-146, that is not
    this library's tokenizer) makes of the same text.  The text carries every quirk of the format between its generated lines."""
    import synthdata as synth
    from tests.helpers import gaf_quirks_text
    if piece is not None:
        set_opt(eng, "gaf_piece_bytes", piece)     # several pieces, joined on the device
    sset = synth.make_set(78, 3, 4, 30000, 60000, with_ids=True)
    p1 = tmp_path / "gen.gaf"
    synth.write_gaf(sset.reads, p1)
    gen = p1.read_bytes()
    cut = gen.index(b"\n", len(gen) // 2) + 1
    p = tmp_path / "mixed.gaf"
    p.write_bytes(gen[:cut] + gaf_quirks_text() + b"\n" + gen[cut:])
    eng.upload_db(sset.species)
    cols = eng.load_reads_from_gaf(p)
    sp, rc, bs, lm, uq = eng.rcls_profile()
    eng.db_reset()
    eng.trio_nodes_info()
    bases, cov, tb, nab = eng.get_node_abundances()
    a = (cols, sp, (rc, bs, lm, uq), bases, cov, tb, nab)
    # ... and the reads of the oracle's reading of the same text (oracle/gaf_reader.py), uploaded as packed arrays
    from oracle import gaf_reader
    w = gaf_reader.packed(p.read_bytes())
    for k in a[0]:
        assert np.array_equal(a[0][k], w[k]), ("oracle", k)
    eng.upload_reads(w["step_off"], w["node_id"], w["pstart"], w["pend"], w["qlen"], w["mapq"], flags=w["flags"])
    sp, *_ = eng.rcls_profile()
    eng.db_reset()
    eng.trio_nodes_info()
    bases, cov, tb, nab = eng.get_node_abundances()
    assert np.array_equal(sp, a[1])
    assert np.array_equal(bases, a[3]) and np.array_equal(cov, a[4]) and np.array_equal(tb, a[5]) and nab == a[6]


@pytest.mark.gpu
@pytest.mark.parametrize("piece", [None, "200000", "97"])
def test_device_gaf_tokenizer_equals_host_tokenizer(eng, tmp_path, piece, set_opt):
    """pantax_hip_gaf_load_device (GAF text tokenised by HIP kernels) gives the arrays of the host tokenizer bit for
    bit: a generated GAF plus every quirk of the format contract (comments, '*' nulls, CRLF, ragged and empty lines,
    no trailing newline, overflowing numbers, 13+ fields, digits inside non-numeric fields)."""
    from pantax_amd import io as pio
    import synthdata as synth
    # texts of 4 GiB and more are tokenised in pieces cut at line ends and joined on the device; a small piece size
    # sends these small files through that path (97 bytes: nearly every line of the quirks file is its own piece)
    if piece is not None:
        set_opt(eng, "gaf_piece_bytes", piece)
    sset = synth.make_set(77, 3, 4, 20000 if piece != "97" else 300, 60000, with_ids=True)
    p1 = tmp_path / "gen.gaf"
    synth.write_gaf(sset.reads, p1)
    p2 = tmp_path / "quirks.gaf"
    p2.write_bytes(
        b"@HD\tVN:1.0\n"
        b"r1\t150\t0\t150\t+\t>12<7>300\t400\t3\t153\t150\t150\t60\tNM:i:0\n"
        b"r2\t150\t0\t150\t+\t*\t*\t*\t*\t*\t*\t255\n"
        b"r3\t100\t0\t100\t+\t<5\t30\t20\t10\t100\t100\t*\r\n"
        b"\n"
        b"\r\n"
        b"r5\t99999999999\t0\t1\t+\t>4294967296>7\t1\t99999999999\t5\t1\t1\t300\ta\tb\tc\n"
        b"r6\tx12\t0\t1\t+\t>1>2\t12x\t3\t4\t1\t1\t7\n"
        b"r7\t10\t0\t10\t+\tabc>>9<<10zz11\t5\t\t6\n"
        b"@ comment in the middle\n"
        b"r8\n"
        b"r9\t90\t0\t90\t+\t>8>9\t200\t0\t90")
    from oracle import gaf_reader
    from tests.helpers import gaf_quirks_text
    p3 = tmp_path / "quirks2.gaf"
    p3.write_bytes(gaf_quirks_text())
    for p in (p1, p2, p3):
        if piece == "97" and p is not p2:
            continue                      # their lines are longer than the piece: refused, see below
        host = pio.load_gaf(p, n_threads=3)
        dev = pio.load_gaf(p, engine=eng)
        want = gaf_reader.packed(p.read_bytes())      # the reading of the format that is not this repo's tokenizer (oracle/gaf_reader.py)
        for k in host:
            assert np.array_equal(host[k], dev[k]), (p.name, k)
            assert np.array_equal(want[k], dev[k]), (p.name, "oracle", k)
    # every alignment of the lines against the tokenizer's 8-byte window (TxtWin): the quirks behind a comment line of 0 .. 16 bytes, plus fields of 7, 8 and
    # 9 bytes, empty fields side by side and a tab as a line's last byte
    body = p2.read_bytes() + b"\nq1\t1234567\t0\t1\t+\t>12345678>123456789\t12345678\t1\t123456789\t1\t1\t60\n" \
                             b"q2\t\t\t\t\t\t\t\t\t\t\t\nq3\t8\t0\t8\t+\t>1\t9\t0\t8\t8\t8\t60\t\nq4\t8\t0\t8\t+\t>1>2>3>4>5>6>7>8>9>10>11>12>13>14>15>16>17\t9\t0\t8\t8\t8\t0"
    for k in range(17):
        pk = tmp_path / ("shift%d.gaf" % k)
        pk.write_bytes(b"@" + b"x" * k + b"\n" + body)
        dev = pio.load_gaf(pk, engine=eng)
        want = gaf_reader.packed(pk.read_bytes())
        for key in want:
            assert np.array_equal(want[key], dev[key]), (k, key)
    if piece == "97":
        from pantax_amd.engine import PantaxHipError
        with pytest.raises(PantaxHipError):
            pio.load_gaf(p1, engine=eng)   # a line longer than a piece
    empty = tmp_path / "empty.gaf"
    empty.write_bytes(b"")
    assert pio.load_gaf(empty, engine=eng)["step_off"].tolist() == [0]
    only_comments = tmp_path / "c.gaf"
    only_comments.write_bytes(b"@a\n@b\n")
    d = pio.load_gaf(only_comments, engine=eng)
    assert d["step_off"].tolist() == [0] and len(d["pstart"]) == 0


@pytest.mark.gpu
def test_resident_reads_from_gaf_equal_uploaded_reads(eng, tmp_path, set_opt):
    """pantax_hip_reads_load_gaf (file -> device tokenizer -> resident reads, walks never on the host) gives the same
    binning, counters, coverage histogram and trio bases as uploading the host-tokenised arrays; drop flags can be
    replaced in place."""
    from pantax_amd import io as pio
    import synthdata as synth
    set_opt(eng, "gaf_piece_bytes", "1000000")   # the resident form through the piece-wise tokenizer as well
    sset = synth.make_set(78, 3, 4, 30000, 80000)
    p1 = tmp_path / "gen.gaf"
    synth.write_gaf(sset.reads, p1)
    eng.upload_db(sset.species)
    host = pio.load_gaf(p1)
    flags = (np.arange(len(host["qlen"])) % 7 == 0).astype(np.uint8)

    def run():
        sp, *cnt = eng.rcls_profile()
        eng.db_reset(); eng.trio_nodes_info(fetch=False)
        b, c, t, n = eng.get_node_abundances()
        return sp, cnt, b, c, t, n
    eng.upload_reads(host["step_off"], host["node_id"], host["pstart"], host["pend"], host["qlen"], host["mapq"], host["flags"])
    ref = run()
    eng.upload_reads(host["step_off"], host["node_id"], host["pstart"], host["pend"], host["qlen"], host["mapq"], flags)
    ref_f = run()
    cols = eng.load_reads_from_gaf(p1)
    assert np.array_equal(cols["qlen"], host["qlen"]) and np.array_equal(cols["mapq"], host["mapq"]) and np.array_equal(cols["flags"], host["flags"])
    got = run()
    eng.set_read_flags(flags)
    got_f = run()
    for a, b in ((ref, got), (ref_f, got_f)):
        assert np.array_equal(a[0], b[0])
        for x, y in zip(a[1], b[1]):
            assert np.array_equal(x, y)
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and a[5] == b[5]
    assert not np.array_equal(ref[2], ref_f[2])   # the flags did drop something


@pytest.mark.gpu
def test_cli_binary_matches_library_call(world):
    """pantax_amd/lib/pantax-hip (the stand-alone front end of the pipeline seam) writes the same tables as the
    library call, for the default .bin graphs and the zstd ones; bad usage exits non-zero."""
    import subprocess
    sset, root, db, gaf, eng = world
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    assert os.path.exists(exe)
    if not os.path.exists(db / "species_graph_info" / (sset.species[0].name + ".bin.zst")):
        import pyarrow as pa
        for f in os.listdir(db / "species_graph_info"):
            if f.endswith(".bin"):
                (db / "species_graph_info" / (f + ".zst")).write_bytes(pa.Codec("zstd").compress(open(db / "species_graph_info" / f, "rb").read(), asbytes=True))
    ref = root / "wd_cli_ref"
    ref.mkdir()
    cwd = os.getcwd()
    os.chdir(str(ref))
    try:
        eng.profile(str(db), str(ref), str(gaf), zip="serialize")
    finally:
        os.chdir(cwd)
    for name, extra in (("wd_cli", []), ("wd_cli_zst", ["--zip", "zstd"])):
        wd = root / name
        wd.mkdir()
        r = subprocess.run([exe, "-db", str(db), "-T", str(wd), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0"] + extra,
                           cwd=str(wd), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        for f in ("species_abundance.txt", "strain_abundance.txt"):
            assert open(wd / f).read() == open(ref / f).read(), (name, f)
    r = subprocess.run([exe, "-db", str(db)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    r = subprocess.run([exe, "-db", str(db), "-T", str(root), "--gaf", str(root / "nope.gaf"), "--species"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "valid file path" in r.stderr


@pytest.mark.gpu
def test_cli_rank_whose_peer_never_starts_gives_up_at_its_deadline(world):
    """--ranks 2 --rank 0 with nobody behind rank 1: the RCCL bootstrap is non-blocking and polled (cli/rccl_comm.hpp), so rank 0 aborts the
    communicator at --comm-timeout and exits non-zero by itself -- no launcher-side timeout needed, nothing hangs."""
    import subprocess
    import time
    sset, root, db, gaf, eng = world
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wd = root / "wd_lonely_rank"
    wd.mkdir()
    t0 = time.time()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wd), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0",
                        "--ranks", "2", "--rank", "0", "--device", "0", "--comm-timeout", "6", "--comm-nonce", "4242"],
                       cwd=str(wd), capture_output=True, text=True, timeout=180)
    dt = time.time() - t0
    assert r.returncode != 0, r.stderr
    assert "deadline" in r.stderr or "bootstrap" in r.stderr, r.stderr
    assert dt < 120, dt
    assert not os.path.exists(wd / "strain_abundance.txt")


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n,piece", [(1, 200, None), (2, 5000, None), (3, 40000, None), (2, 5000, "100000"), (4, 300, "4000")])
def test_device_gaf_filter_equals_oracle(eng, tmp_path, seed, n, piece, set_opt):
    """pantax_hip_gaf_filter == filter_max_alignment_mt (gaf_filter.rs:44-97) as restated by the oracle: the written
    lines are exactly the oracle's, in file order, with line ends normalised the way BufRead::lines + writeln! do."""
    from oracle import oracle as orc
    from tests.helpers import make_longread_gaf
    if piece is not None:   # texts of 4 GiB and more go through in pieces; the alignments of a read land in different ones
        set_opt(eng, "gaf_piece_bytes", piece)
    txt = make_longread_gaf(seed, n)
    gp = tmp_path / "gfa_mapped.gaf"
    gp.write_bytes(txt)
    n_lines, n_rec, n_written = eng.gaf_filter(str(gp))
    keep, nrec = orc.gaf_filter(txt)
    lines = txt.split(b"\n")
    if txt.endswith(b"\n"):
        lines = lines[:-1]
    assert n_lines == len(lines) == len(keep) and n_rec == nrec and n_written == int(keep.sum()) > 0
    exp = b"".join((lines[i][:-1] if lines[i].endswith(b"\r") else lines[i]) + b"\n" for i in np.nonzero(keep)[0])
    out = tmp_path / "gfa_mapped_filtered.gaf"          # <stem>_filtered.gaf beside the input (gaf_filter.rs:46-49)
    assert out.read_bytes() == exp
    # explicit output path; filtering the filtered file changes nothing (idempotence)
    out2 = tmp_path / "twice.gaf"
    n2 = eng.gaf_filter(str(out), str(out2))
    assert n2[0] == n_written and n2[2] == n_written and out2.read_bytes() == exp
    if seed == 2 and piece is None:   # the stand-alone front end
        import subprocess
        exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
        out3 = tmp_path / "cli.gaf"
        r = subprocess.run([exe, "--filter-only", str(gp), str(out3)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "%d written" % n_written in r.stdout, r.stderr
        assert out3.read_bytes() == exp


@pytest.mark.gpu
def test_device_gaf_filter_edge_inputs(eng, tmp_path):
    from pantax_amd.engine import PantaxHipError
    empty = tmp_path / "empty.gaf"
    empty.write_bytes(b"")
    assert eng.gaf_filter(str(empty)) == (0, 0, 0) and (tmp_path / "empty_filtered.gaf").read_bytes() == b""
    junk = tmp_path / "junk.gaf"
    junk.write_bytes(b"\n\n@x\nnot\ta\trecord\n")
    assert eng.gaf_filter(str(junk)) == (4, 0, 0)
    # every alignment of the lines against the field splitter's 8-byte window: the same records behind a first line of 0 .. 8 bytes
    from oracle import oracle as orc
    from tests.helpers import make_longread_gaf
    base = make_longread_gaf(9, 60)
    for k in range(9):
        txt = b"#" * k + b"\n" + base
        gp = tmp_path / ("shift%d.gaf" % k)
        gp.write_bytes(txt)
        n_lines, n_rec, n_written = eng.gaf_filter(str(gp))
        keep, nrec = orc.gaf_filter(txt)
        lines = txt.split(b"\n")
        if txt.endswith(b"\n"):
            lines = lines[:-1]
        assert (n_lines, n_rec, n_written) == (len(lines), nrec, int(keep.sum()))
        exp = b"".join((lines[i][:-1] if lines[i].endswith(b"\r") else lines[i]) + b"\n" for i in np.nonzero(keep)[0])
        assert (tmp_path / ("shift%d_filtered.gaf" % k)).read_bytes() == exp
    with pytest.raises(PantaxHipError):
        eng.gaf_filter(str(tmp_path / "missing.gaf"))


@pytest.mark.gpu
def test_graph_images_roundtrip_and_file_seam(world, tmp_path):
    """device-ready images (the graph in the kernels' layouts; format 3 no longer stores the unique-trio index -- the device
    rebuilds it faster than PCIe delivers it, db_image.cpp).  A db loaded from images has the trio table of the db it was saved from
    (built on the device from the streamed walks) and gives the same strain step; the file seam writes them (image_cache 2), uses them
    (image_cache 1: no graph parse), and falls back to the graph file of a species whose image is truncated or stale."""
    from pantax_amd.engine import Engine, metrics_to_dicts
    sset, root, db, gaf, eng0 = world
    eng = Engine(0)
    try:
        rd = sset.reads
        eng.upload_db(sset.species)
        eng.upload_packed(rd)
        trio_a = eng.trio_nodes_info()
        sp, rc, bs, lm, uq = eng.rcls_profile()
        keep, absolute, _ = eng.species_profiling((rc, bs, lm, uq), sset.avg_len())
        cov_a = eng.get_node_abundances()
        met_a = metrics_to_dicts(eng.strain_profiling(absolute, species_active=keep)[0], eng.H)
        paths = [str(tmp_path / (g.name + ".hipdb")) for g in sset.species]
        eng.save_images(paths, [hn for g in sset.species for hn in g.hap_names])
        eng.load_images(paths, [g.range_start for g in sset.species], [g.range_end for g in sset.species], sset.species)
        trio_b = eng.trio_nodes_info()                       # built from the walks the images delivered
        for a, b in zip(trio_a, trio_b):
            assert np.array_equal(a, b)
        eng.rcls_profile()
        cov_b = eng.get_node_abundances()
        for a, b in zip(cov_a[:3], cov_b[:3]):
            assert np.array_equal(a, b)
        met_b = metrics_to_dicts(eng.strain_profiling(absolute, species_active=keep)[0], eng.H)
        assert met_a == met_b
        # a truncated image is refused by the loader
        bad = tmp_path / "bad.hipdb"
        bad.write_bytes(open(paths[0], "rb").read()[:-40])
        from pantax_amd.engine import PantaxHipError
        with pytest.raises(PantaxHipError):
            eng.load_images([str(bad)] + paths[1:], [g.range_start for g in sset.species], [g.range_end for g in sset.species], sset.species)
    finally:
        eng.close()
    # ---- file seam
    exp_species, exp_strain, _ = _oracle_tables(sset)
    import shutil
    db2 = root / "db_img"
    shutil.copytree(db, db2)
    cwd = os.getcwd()

    def run(name, **kw):
        wd = root / name
        wd.mkdir()
        os.chdir(str(wd))
        try:
            eng0.profile(str(db2), str(wd), str(gaf), **kw)
        finally:
            os.chdir(cwd)
        _check_outputs(str(wd), sset, exp_species, exp_strain)
        return wd
    imgs = [db2 / "species_graph_info" / (g.name + ".hipdb") for g in sset.species]
    run("wd_img0", image_cache=1)                            # no images yet: parsed, none written
    assert not any(p.exists() for p in imgs)
    run("wd_img_write", image_cache=2)
    kept = [p for p in imgs if p.exists()]
    assert kept                                              # one per species that went through the strain step
    ref = run("wd_img_read", image_cache=1)
    kept[0].write_bytes(kept[0].read_bytes()[:1000])         # damaged image: the run falls back to the graph files
    run("wd_img_damaged", image_cache=1)
    run("wd_img_rewrite", image_cache=2)                     # parsed again, and the images are written afresh
    assert kept[0].stat().st_size > 1000
    run("wd_img_read2", image_cache=1)
    for f in ("species_abundance.txt", "strain_abundance.txt"):
        assert open(ref / f).read() == open(root / "wd_img_write" / f).read()


@pytest.mark.gpu
@pytest.mark.parametrize("world_size", [2, 3])
def test_profile_seam_sharded_over_ranks(world, world_size):
    """The file seam with world_size > 1 (one process per GPU in production; here the ranks are threads with their own
    ctx on the one GPU and a barrier-based sum as the all-reduce): every rank handles its share of the species (longest-processing-time packing),
    the two global sums and the rows meet through the callback and the part files, rank 0 writes the same tables as a
    single-rank run."""
    import threading
    from pantax_amd.engine import Engine
    sset, root, db, gaf, eng0 = world
    exp_species, exp_strain, _ = _oracle_tables(sset)
    wd = root / ("wd_shard%d" % world_size)
    wd.mkdir()
    bar = threading.Barrier(world_size)
    slots = [None] * world_size
    total = [None]

    def make_allreduce(rank):
        def allreduce(buf):
            slots[rank] = buf.copy()
            if bar.wait() == 0:
                total[0] = np.sum(slots, axis=0)
            bar.wait()
            buf[:] = total[0]
            bar.wait()
        return allreduce
    errs = []

    def run(rank):
        eng = Engine(0)
        try:
            eng.profile(str(db), str(wd), str(gaf), rank=rank, world_size=world_size, allreduce=make_allreduce(rank),
                        out_binning_file=str(wd / "reads_classification.tsv"))
        except Exception as e:   # noqa: BLE001
            errs.append((rank, e))
            bar.abort()
        finally:
            eng.close()
    cwd = os.getcwd()

    def launch(fn):
        os.chdir(str(wd))
        try:
            ths = [threading.Thread(target=fn, args=(r,)) for r in range(world_size)]
            for t in ths:
                t.start()
            for t in ths:
                t.join(timeout=300)
        finally:
            os.chdir(cwd)
        assert not errs, errs
    launch(run)
    _check_outputs(str(wd), sset, exp_species, exp_strain)
    assert os.path.exists(wd / "ori_strain_abundance.txt") and os.path.exists(wd / "reads_classification.tsv")
    assert not [f for f in os.listdir(wd) if ".part" in f]
    # the resume path over ranks (profile.rs:3365-3417): the strain table is gone, the species table and the report stay ->
    # rank 0's view of the work directory decides for everybody, the strain level is redone from the saved binning
    os.remove(wd / "strain_abundance.txt")
    before = os.path.getmtime(wd / "species_abundance.txt")

    def run_resume(rank):
        eng = Engine(0)
        try:
            eng.profile(str(db), str(wd), str(gaf), rank=rank, world_size=world_size, allreduce=make_allreduce(rank))
        except Exception as e:   # noqa: BLE001
            errs.append((rank, e))
            bar.abort()
        finally:
            eng.close()
    launch(run_resume)
    assert os.path.getmtime(wd / "species_abundance.txt") == before
    _check_outputs(str(wd), sset, exp_species, exp_strain)
    # the rows are in the one-process order as well: same file as the single-rank run apart from the last digits of the sums
    one = root / "wd_bin"
    if (one / "strain_abundance.txt").exists():
        a = [l.split("\t")[:3] for l in open(one / "strain_abundance.txt")]
        b = [l.split("\t")[:3] for l in open(wd / "strain_abundance.txt")]
        assert a == b
    # a missing callback is refused
    from pantax_amd.engine import PantaxHipError
    with pytest.raises(PantaxHipError):
        eng0.profile(str(db), str(wd), str(gaf), rank=0, world_size=2, force=True)


@pytest.mark.gpu
def test_device_gaf_filter_and_sampler_against_fixtures(eng, tmp_path, golden_dir):
    """The same fixtures through the device filter and the library's sampler (no oracle call on this path)."""
    import json
    from pantax_amd.engine import Engine
    g = json.load(open(os.path.join(golden_dir, "gaf_filter.json")))
    txt = g["text"].encode("latin-1")
    gp = tmp_path / "fx.gaf"
    gp.write_bytes(txt)
    n_lines, n_rec, n_written = eng.gaf_filter(str(gp), str(tmp_path / "fx_out.gaf"))
    lines = txt.split(b"\n")
    if txt.endswith(b"\n"):
        lines = lines[:-1]
    exp = b"".join((lines[i][:-1] if lines[i].endswith(b"\r") else lines[i]) + b"\n" for i in g["kept_lines"])
    assert n_rec == g["n_records"] and n_written == len(g["kept_lines"]) and (tmp_path / "fx_out.gaf").read_bytes() == exp
    z = json.load(open(os.path.join(golden_dir, "sampler_positions.json")))
    for c in z["cases"]:
        pos = np.nonzero(Engine.sample_ranks(c["n"], c["amount"], seed=c["seed"]))[0]
        assert pos[:8].tolist() == c["first"] and pos[-4:].tolist() == c["last"] and int(pos.sum()) == c["sum"]


@pytest.mark.gpu
def test_profile_seam_sharded_failure_reaches_every_rank(world):
    """One rank cannot load a graph of its shard: it reports the failure through the exchange, every rank returns an
    error (nobody is left waiting in the all-reduce) and no strain table appears."""
    import shutil
    import threading
    from pantax_amd.engine import Engine, PantaxHipError
    sset, root, db, gaf, eng0 = world
    db2 = root / "db_broken"
    shutil.copytree(db, db2)
    exp_species, exp_strain, _ = _oracle_tables(sset)
    profiled = sorted({r[0] for r in exp_strain})                 # species that reach the strain level, selection order = species table order
    sel_order = [r[0] for r in exp_species if r[0] in profiled]
    victim = sel_order[1]                                          # one of the two ranks owns it
    for sub, ext in (("species_graph_info", ".bin"), ("species_gfa", ".gfa")):
        os.remove(db2 / sub / (victim + ext))
    wd = root / "wd_shard_fail"
    wd.mkdir()
    bar = threading.Barrier(2)
    slots, total, errs = [None, None], [None], {}

    def make_allreduce(rank):
        def allreduce(buf):
            slots[rank] = buf.copy()
            if bar.wait(timeout=120) == 0:
                total[0] = np.sum(slots, axis=0)
            bar.wait(timeout=120)
            buf[:] = total[0]
            bar.wait(timeout=120)
        return allreduce

    def run(rank):
        eng = Engine(0)
        try:
            eng.profile(str(db2), str(wd), str(gaf), rank=rank, world_size=2, allreduce=make_allreduce(rank))
        except PantaxHipError as e:
            errs[rank] = str(e)
        finally:
            eng.close()
    cwd = os.getcwd()
    os.chdir(str(wd))
    try:
        ths = [threading.Thread(target=run, args=(r,)) for r in range(2)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(timeout=300)
            assert not t.is_alive()
    finally:
        os.chdir(cwd)
    assert set(errs) == {0, 1}
    own = [r for r in (0, 1) if "does not exist" in errs[r]]
    assert len(own) == 1 and "another rank failed" in errs[1 - own[0]]
    assert not os.path.exists(wd / "strain_abundance.txt") and os.path.exists(wd / "species_abundance.txt")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_profile_seam_vs_literal_python_restatement(tmp_path, k):
    """Files in, tables out (pantax_hip_profile) against the fixtures of oracle/ref_literal_strain.py -- the literal Python
    reading of the reference, LP by SciPy-HiGHS: the DB and the GAF are written from the fixture (`*` where it holds a null),
    the two tables must hold the literal reading's rows.  Case 3 has duplicate read ids (kept inside one species, dropped
    across two) and null read_start rows (counted in the species table, dropped at the strain level): profile.rs:361-463."""
    import synthdata as synth
    from pantax_amd.engine import Engine
    from tests.helpers import load_literal_strain_case, write_literal_gaf
    j, sset = load_literal_strain_case(k)
    a, ex = j["args"], j["expect"]
    db = tmp_path / "db"
    db.mkdir()
    synth.write_db(sset, str(db))
    gaf = tmp_path / "reads.gaf"
    write_literal_gaf(j, str(gaf))
    wd = tmp_path / "wd"
    wd.mkdir()
    eng = Engine(0)
    cwd = os.getcwd()
    os.chdir(str(wd))
    try:
        eng.profile(str(db), str(wd), str(gaf), fr=a["fr"], fc=a["fc"], sr=a["sr"], sd=a["sd"], min_species_abundance=a["min_species_abundance"],
                    min_cov=a["min_cov"], min_depth=a["min_depth"], shift=a["shift"], filtered=a["filtered"], sample_nodes=0,
                    solver_semantics=1 if a.get("solver") == "highs" else 0)      # (case 4: --solver highs, profile.rs:2865-2879)
    finally:
        os.chdir(cwd)
        eng.close()
    exp_species = [(r["species_taxid"], r["predicted_abundance"], r["predicted_coverage"]) for r in ex["species_profile"]]
    key = {"path_base_cov": "path_cov_ratio", "unique_trio_fraction": "unique_trio_nodes_fraction", "uniq_trio_cov_mean": "frequencies_mean",
           "first_sol": "first_sol", "strain_cov_diff": "divergence", "total_cov_diff": "total_cov_diff"}
    exp_strain = []
    for e in ex["final_rows"]:
        m = [m for m in ex["per_species"][e["species_taxid"]]["metrics"] if m["hap_id"] == e["hap_id"]][0]
        exp_strain.append((e["species_taxid"], e["hap_id"], e["predicted_coverage"], e["predicted_abundance"], {c: m[f] for c, f in key.items()}))
    _check_outputs(str(wd), sset, exp_species, exp_strain)


@pytest.mark.gpu
def test_trio_index_prefetch_serves_the_next_step_only(eng):
    """pantax_hip_trio_index_prefetch: the index build of the coming run started ahead of it (before the reads are uploaded) -- the
    step that follows gives the tables of a plain step bit for bit and consumes the prefetch; the step after it rebuilds again;
    a prefetch followed by a db reset is not used."""
    import synthdata as synth
    sset = synth.make_set(41, 4, 8, 60000, 30000, present_frac=0.5)
    avg = sset.avg_len()
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    def snap(o):      # the step's outputs live in buffers the engine reuses: copies
        return (o[0].copy(), o[1].copy(), bytes(memoryview(o[2])), str([(i.n_candidates, i.status1, i.iters1, i.n_rows, i.n_patterns, i.obj1, i.obj2) for i in o[3]]),
                o[4].copy())

    def same(a, b):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3] and np.array_equal(a[4], b[4])

    ref = snap(eng.profile_step(avg))
    assert ref[0].any()
    eng.trio_index_prefetch()
    eng.upload_packed(sset.reads)            # the "load" of the run the prefetch belongs to
    same(snap(eng.profile_step(avg)), ref)
    same(snap(eng.profile_step(avg)), ref)   # no prefetch in front of this one: it builds its own
    eng.trio_index_prefetch()
    eng.trio_index_prefetch()                # twice in a row: the second replaces the first
    same(snap(eng.profile_step(avg)), ref)
    eng.trio_index_prefetch()
    eng.upload_db(sset.species)              # a new db: nothing of the prefetch survives
    eng.upload_packed(sset.reads)
    same(snap(eng.profile_step(avg)), ref)
