"""Direct tests of the device-side graph load and of the image format 4 (db_image.cpp, stage_db.hip, api_core.cpp db_upload_arrays), bit-exact.

pantax_hip_db_save_images downloads d_node_len, d_path_nodes and the two ends of d_bit_off, so it is the read-back of every upload route.  The
reference is the tests' own codec (tests/hipdb_codec.py, numpy, pinned on the host by tests/test_db_image_codec.py): the library's encoder must
write its canonical bytes, and walks_unpack_kernel / lens_widen_kernel must deliver, element by element, what it decodes -- over the corpus of
tests/db_image_corpus.py (block and round borders, the width thresholds, u16 / u32 lengths, thousands of species inside one wave's stretch).

Not covered: a delta of 2^31 or more, the 32-bit wrap of the zigzag.  It needs a species of more than 2^31 nodes."""
import os
import shutil

import numpy as np
import pytest

from tests import db_image_corpus as corp
from tests import hipdb_codec as codec

pytestmark = pytest.mark.gpu

E_INVALID, E_IO = -1, -6
NAMES = sorted(corp.small_corpus()) + ["mixed"]


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def canon(tmp_path_factory):
    """name -> (db, paths of the canonical images the tests' codec writes, their bytes); made once per db"""
    cache = {}
    dbs = {}

    def get(name):
        if name not in cache:
            if not dbs:
                dbs.update(corp.corpus())
            db = dbs[name]
            d = tmp_path_factory.mktemp("canon_" + name)
            paths = _write(db, d)
            cache[name] = (db, paths, [open(p, "rb").read() for p in paths])
        return cache[name]
    return get


def _write(db, d, per_species=None, **kw):
    paths = []
    for i, g in enumerate(db):
        k = dict(kw)
        if per_species is not None:
            k.update(per_species(i, g))
        paths.append(codec.write_image(os.path.join(str(d), g.name + ".hipdb"), g.node_len, g.path_off, g.path_nodes, g.hap_names, g.L, **k))
    return paths


def _ranges(db):
    return [g.range_start for g in db], [g.range_end for g in db]


def _save(eng, db, d):
    os.makedirs(str(d), exist_ok=True)
    paths = [os.path.join(str(d), g.name + ".hipdb") for g in db]
    eng.save_images(paths, [hn for g in db for hn in g.hap_names])
    return paths


def _load(eng, db, paths):
    rs, re = _ranges(db)
    eng.load_images(paths, rs, re, db)


def _check_saved(paths, db, canon_bytes):
    """what the device held, read back: the graph of every species, and the very bytes of the canonical image"""
    for p, g, cb in zip(paths, db, canon_bytes):
        raw = open(p, "rb").read()
        if raw == cb:                                    # (the codec's own read(write(x)) == x is pinned on the host)
            continue
        img = codec.read_image(p)
        assert (img.V, img.H, img.P) == (len(g.node_len), len(g.hap_names), len(g.path_nodes)), g.name
        assert np.array_equal(img.node_len, g.node_len), g.name
        assert np.array_equal(img.path_off, g.path_off), g.name
        bad = np.nonzero(img.path_nodes != g.path_nodes)[0]
        assert len(bad) == 0, "%s: walk position %d is %d, expected %d (%d differ)" % (g.name, bad[0], img.path_nodes[bad[0]], g.path_nodes[bad[0]], len(bad))
        assert img.names == g.hap_names, g.name
        assert img.L == g.L, (g.name, img.L, g.L)
        assert img.len16 == (int(g.node_len.max()) < 65536), g.name
        assert np.array_equal(img.widths, codec.minimal_widths(g.path_nodes)), g.name
        assert raw == cb, "%s: same content, other bytes" % g.name


@pytest.mark.parametrize("name", NAMES)
def test_encoder_and_routes(eng, canon, name, tmp_path):
    """upload_db -> save_images: every species' image holds the graph that went in (lengths, offsets, walks, names, V, H, P), L is the species' own
    sum, LEN16 is set iff the maximum length is below 65536, and the file is byte-identical to the codec's canonical output.  upload_db_flat and
    load_images of the same db save the same bytes."""
    db, cpaths, cbytes = canon(name)
    eng.upload_db(db)
    saved = _save(eng, db, tmp_path / "parts")
    _check_saved(saved, db, cbytes)
    for g, p in zip(db, saved):                          # L and the LEN16 flag, read from the header of the files the library wrote
        hdr = open(p, "rb").read(48)
        flags, L = np.frombuffer(hdr, dtype="<u4", count=1, offset=12)[0], np.frombuffer(hdr, dtype="<u8", count=1, offset=40)[0]
        assert int(L) == int(g.node_len.sum()) and bool(flags & 1) == (int(g.node_len.max()) < 65536)
    eng.upload_db_flat(db)
    _check_saved(_save(eng, db, tmp_path / "flat"), db, cbytes)
    _load(eng, db, cpaths)
    _check_saved(_save(eng, db, tmp_path / "images"), db, cbytes)


@pytest.mark.parametrize("variant", ["w2", "w4", "wmixed", "len32", "all"])
@pytest.mark.parametrize("name", NAMES)
def test_decoder_kernels(eng, canon, name, variant, tmp_path):
    """load_images of valid non-canonical files -- every block at least 2 bytes wide, every block 4 bytes, widths mixed at random, u32 lengths where
    u16 would do, and (all) widths and length types mixed species by species, which puts u16 and u32 species and all three widths into one
    upload -- then save_images: the device held exactly what the numpy decode of the input gives (the canonical load is in test_encoder_and_routes)."""
    db, _, cbytes = canon(name)
    rng = np.random.default_rng(99)
    if variant == "w2":
        paths = _write(db, tmp_path, widths=2)
    elif variant == "w4":
        paths = _write(db, tmp_path, widths=4)
    elif variant == "wmixed":
        paths = _write(db, tmp_path, per_species=lambda i, g: dict(widths=corp.mixed_widths(rng, codec.minimal_widths(g.path_nodes))))
    elif variant == "len32":
        paths = _write(db, tmp_path, len16=False)
    else:
        paths = _write(db, tmp_path, per_species=lambda i, g: dict(widths=corp.mixed_widths(rng, codec.minimal_widths(g.path_nodes)),
                                                                   len16=None if i % 3 else False))
    _load(eng, db, paths)
    _check_saved(_save(eng, db, tmp_path / "out"), db, cbytes)


def test_bit_offsets_beyond_2_32(eng, tmp_path):
    """Nodes of 1e9 bases and more: the cumulative bases reach 2^32 exactly on a species border and cross 2^33 inside a node of the next species.  Every
    image's L is its species' own sum, and coverage lands on the right nodes behind the crossings: one-step reads give bases = covered = pend - pstart
    on their node (distinct stretches), a read over a whole node covers node_len bases (the full-node flag), every other node stays 0.  The expectations are written
    out here: the C oracle keeps a byte per base."""
    G = 1000000000
    specs = [([G, G, G, G, (1 << 32) - 4 * G], [[0, 1, 2, 3, 4], [4, 0]]),                        # sums to 2^32: the border lies on the crossing
             ([3 * G, 2 * G, G, 1000, 77], [[0, 1, 2, 3, 4], [1, 3]]),                            # 2^33 lies inside node 1 (2^32 + 3e9 .. + 5e9)
             ([500, 4294967290, 300], [[0, 1, 2]])]
    db = corp.make_db(specs, "big")
    assert db[0].L == 1 << 32 and (1 << 32) + 3 * G < (1 << 33) < (1 << 32) + 5 * G
    eng.upload_db(db)
    paths = _save(eng, db, tmp_path)
    for p, g in zip(paths, db):
        img = codec.read_image(p)
        assert img.L == g.L and not img.len16 and np.array_equal(img.node_len, g.node_len) and np.array_equal(img.path_nodes, g.path_nodes)
    _load(eng, db, paths)                                                                         # the same through the u32-length image route
    for p, q in zip(paths, _save(eng, db, tmp_path / "again")):
        assert open(p, "rb").read() == open(q, "rb").read()
    # (global node id, pstart, pend) of one-step reads; global ids are 1-based, species after species
    n0 = [g.range_start for g in db]
    reads = [(n0[0] + 4, 10, 5010),                     # the last node in front of 2^32
             (n0[1] + 0, 0, 4000),                      # the first node behind the species border = bit 2^32
             (n0[1] + 0, 2999990000, 2999999999),
             (n0[1] + 1, 1294967290 - 3000, 1294967290 + 3000),     # straddles bit 2^33 inside the node (2^33 - 2^32 - 3e9 = 1294967296)
             (n0[1] + 1, 1999990000, 2 * G),            # up to the node's last base
             (n0[1] + 3, 0, 1000),                      # a whole node behind both crossings
             (n0[1] + 4, 5, 70),
             (n0[2] + 1, 4294960000, 4294967290),       # the end of a node of 2^32 - 6 bases
             (n0[2] + 2, 0, 300)]                       # a whole node, the last of the db
    step_off = np.arange(len(reads) + 1)
    eng.upload_reads(step_off, [r[0] for r in reads], [r[1] for r in reads], [r[2] for r in reads], [r[2] - r[1] for r in reads], [60] * len(reads))
    sp = eng.rcls_profile()[0]
    assert sp.tolist() == [0, 1, 1, 1, 1, 1, 1, 2, 2]
    bases, cov, _, n_abort = eng.get_node_abundances()
    exp = np.zeros(eng.V, dtype=np.int64)
    for nid, ps, pe in reads:
        exp[nid - 1] += pe - ps
    assert n_abort == 0
    assert exp[n0[1] + 3 - 1] == db[1].node_len[3] and exp[n0[2] + 2 - 1] == db[2].node_len[2]   # the two whole-node reads
    assert np.array_equal(bases, exp), (bases.tolist(), exp.tolist())
    assert np.array_equal(cov.astype(np.int64), exp), (cov.tolist(), exp.tolist())


def _refused(eng, code, text, fn):
    from pantax_amd.engine import PantaxHipError
    with pytest.raises(PantaxHipError) as ei:
        fn()
    assert ei.value.code == code and text in str(ei.value), str(ei.value)


def _aftermath(eng, canon, d):
    """the ctx is not left broken: the same engine loads a good db and saves it correctly"""
    db, cpaths, cbytes = canon("thresholds")
    eng.upload_db(db)
    _check_saved(_save(eng, db, os.path.join(str(d), "after_up")), db, cbytes)
    _load(eng, db, cpaths)
    _check_saved(_save(eng, db, os.path.join(str(d), "after_ld")), db, cbytes)


def _block_db():
    """three species of four haplotypes of 256 steps: haplotype h of a species IS its block h (steps of +1: one byte per step)"""
    rng = np.random.default_rng(3)
    return corp.make_db([(rng.integers(1, 50, size=2000), [np.arange(256) + 300 * h + 10 * s for h in range(4)]) for s in range(3)], "rf")


@pytest.mark.parametrize("route", ["plain", "flat", "image"])
def test_refusals_zero_length_and_walk_outside(eng, canon, route, tmp_path):
    """A node of length 0 and a walk that names node id V are refused with a status and a message, through the plain uploads and through an image
    with a valid header and end marker; of two offending haplotypes the error names the smaller index.  The engine then works as before."""
    def up(db, tag):
        if route == "plain":
            eng.upload_db(db)
        elif route == "flat":
            eng.upload_db_flat(db)
        else:
            d = tmp_path / tag
            d.mkdir()
            _load(eng, db, _write(db, d))
    db = _block_db()
    db[1].node_len[1999] = 0
    _refused(eng, E_INVALID, "node of length 0", lambda: up(db, "len0"))
    _aftermath(eng, canon, tmp_path / "a0")
    db = _block_db()
    db[1].path_nodes[3 * 256 + 17] = 2000              # global haplotype 7: node id V
    _refused(eng, E_INVALID, "hap 7 walks a node outside its species graph", lambda: up(db, "walk1"))
    _aftermath(eng, canon, tmp_path / "a1")
    db[2].path_nodes[1 * 256] = 2000                   # and global haplotype 9
    db[1].path_nodes[2 * 256 + 255] = 0xFFFFFFFE       # and 6, the smallest
    _refused(eng, E_INVALID, "hap 6 walks a node outside its species graph", lambda: up(db, "walk3"))
    _aftermath(eng, canon, tmp_path / "a3")
    db[1].path_nodes[2 * 256 + 255] = 1999             # the last node of the graph is inside it
    db[1].path_nodes[3 * 256 + 17] = 1999
    _refused(eng, E_INVALID, "hap 9 walks a node outside its species graph", lambda: up(db, "walk9"))
    _aftermath(eng, canon, tmp_path / "a2")


@pytest.mark.parametrize("width", [0, 3, 8])
def test_refusal_block_of_impossible_width(eng, canon, width, tmp_path):
    """An image whose header, end marker and the two ends of blk_off are valid, with one block whose blk_off difference is 0, 3 or 8: the kernel writes the
    block as 0xFFFFFFFF and the walk check names its haplotype.  No offset leaves the species' own payload.  In every table block 1 (= haplotype 1) of the
    first species is the FIRST block of a width other than 1, 2 or 4, and block 0 decodes to a walk inside the graph (the low bytes of steps of +1 are
    steps of +1 and 0): a kernel that accepted the width under test would move the refusal to a later haplotype."""
    db = _block_db()
    widths, off = {0: ([1, 1, 1, 1], [0, 1, 1, 3, 4]),            # widths 1 0 2 1 (block 2 reads units 1..2 as 2 bytes: garbage, inside)
                   3: ([2, 2, 1, 1], [0, 1, 4, 5, 6]),            # widths 1 3 1 1
                   8: ([4, 4, 1, 1], [0, 1, 9, 10, 10])}[width]   # widths 1 8 1 0
    assert np.diff(off).tolist()[:2] == [1, width] and off[0] == 0 and max(off) == off[-1] == sum(widths)
    paths = _write(db, tmp_path, per_species=lambda i, g: dict(widths=widths, blk_off=off) if i == 0 else dict())
    _refused(eng, E_INVALID, "hap 1 walks a node outside its species graph", lambda: _load(eng, db, paths))
    _aftermath(eng, canon, tmp_path / "after")


def _guard_db():
    """two species of four haplotypes of 256 steps that stay on ONE node each: every delta is 0, so the payload is all zero bytes and decodes to the same
    walk at any width and from any unit"""
    return corp.make_db([(np.full(50, 9), [np.full(256, 5 * h + s) for h in range(4)]) for s in range(2)], "gd")


def test_offset_guard_device(eng, canon, tmp_path):
    """Case A: an interior blk_off entry of the FIRST of two species points into the second species' payload; the table's two ends are consistent, so
    only the kernel can notice.  blk_off 0 1 2 6 4 over a payload of 4 units: block 2 is 4 bytes wide and spans units 2..5 -- two of its own, two of the
    next species (inside the scratch buffer of 8 units; all zero, so it decodes to a walk inside the graph) --, block 3 has a negative width.  Without
    the guard block 2 is read and accepted, and only haplotype 3 is refused; with it the first block that leaves its species' payload is refused: hap 2."""
    db = _guard_db()
    paths = _write(db, tmp_path, per_species=lambda i, g: dict(blk_off=[0, 1, 2, 6, 4]) if i == 0 else dict())
    _refused(eng, E_INVALID, "hap 2 walks a node outside its species graph", lambda: _load(eng, db, paths))
    _aftermath(eng, canon, tmp_path / "after")
    d = tmp_path / "good"                                # (the undamaged pair loads: the shape itself is fine)
    d.mkdir()
    good = _write(db, d)
    _load(eng, db, good)
    for p, q in zip(good, _save(eng, db, tmp_path / "good_out")):
        assert open(p, "rb").read() == open(q, "rb").read()


def test_offset_guard_host(eng, canon, tmp_path):
    """Case B: only the LAST blk_off entry is damaged (3 for a payload of 4 units: the last block would have width 0 and is never read).  The loader
    refuses the file when it opens it, before anything is uploaded; so it does a first entry that is not 0."""
    db = _guard_db()
    for k, off in enumerate(([0, 1, 2, 3, 3], [1, 1, 2, 3, 4])):
        d = tmp_path / ("b%d" % k)
        d.mkdir()
        paths = _write(db, d, per_species=lambda i, g: dict(blk_off=off) if i == 0 else dict())
        _refused(eng, E_IO, "block offsets do not span its payload", lambda: _load(eng, db, paths))
    _aftermath(eng, canon, tmp_path / "after")


def test_good_load_behind_each_host_refusal(eng, tmp_path):
    """test_offset_guard_host looks at the engine once, behind both of its refusals (every other refusal of this file is followed by _aftermath at
    once).  Here the undamaged pair of the same two species is loaded directly behind EACH refused load, on the same engine: the staging ring is free
    again (no lease is left behind by a refused call), and the arrays the device then holds are the codec's, byte for byte."""
    db = _guard_db()
    d = tmp_path / "good"
    d.mkdir()
    good = _write(db, d)
    for k, off in enumerate(([0, 1, 2, 3, 3], [1, 1, 2, 3, 4])):
        b = tmp_path / ("b%d" % k)
        b.mkdir()
        paths = _write(db, b, per_species=lambda i, g: dict(blk_off=off) if i == 0 else dict())
        _refused(eng, E_IO, "block offsets do not span its payload", lambda: _load(eng, db, paths))
        _load(eng, db, good)
        for p, q in zip(good, _save(eng, db, tmp_path / ("out%d" % k))):
            assert open(p, "rb").read() == open(q, "rb").read(), (k, p)


# ---------------------------------------------------------------------------------------------------------------- the file seam
@pytest.fixture(scope="module")
def world(tmp_path_factory, eng):
    """a small set on disk, its images written by a run with image_cache = 2, and the species in the order the seam loads them"""
    import synthdata as synth
    from tests.test_gpu_pipeline import _oracle_tables
    sset = synth.make_set(31, 4, 5, 30000, 30000, present_frac=0.4, single_strain_every=4, with_ids=False)
    root = tmp_path_factory.mktemp("seam")
    db = root / "db"
    db.mkdir()
    synth.write_db(sset, str(db))
    gaf = root / "reads.gaf"
    synth.write_gaf(sset.reads, str(gaf))
    exp_species, exp_strain, _ = _oracle_tables(sset)
    w = dict(sset=sset, root=root, db=db, gaf=gaf, exp=(exp_species, exp_strain))
    _run(eng, w, "wd_plain", db, image_cache=0)
    _run(eng, w, "wd_write", db, image_cache=2)
    order = [r[0] for r in exp_species]                               # species_abundance.txt order = the order of the selection
    w["images"] = [n for n in order if (db / "species_graph_info" / (n + ".hipdb")).exists()]
    assert len(w["images"]) >= 3
    return w


def _run(eng, w, name, db, **kw):
    from tests.test_gpu_pipeline import _check_outputs
    wd = w["root"] / name
    wd.mkdir()
    cwd = os.getcwd()
    os.chdir(str(wd))
    try:
        eng.profile(str(db), str(wd), str(w["gaf"]), **kw)
    finally:
        os.chdir(cwd)
    _check_outputs(str(wd), w["sset"], *w["exp"])
    return wd


def _same_tables(a, b):
    for f in ("species_abundance.txt", "strain_abundance.txt"):
        assert open(a / f, "rb").read() == open(b / f, "rb").read(), f


def _copy_db(w, name):
    db2 = w["root"] / name
    shutil.copytree(w["db"], db2, copy_function=shutil.copy2)         # (an image must not be older than its source: the times are kept)
    return db2


def test_file_seam_writes_canonical_images(world):
    """the images the seam leaves behind are the canonical images of the graphs it loaded from the bincode files"""
    by_name = {g.name: g for g in world["sset"].species}
    for n in world["images"]:
        g = by_name[n]
        img = codec.read_image(str(world["db"] / "species_graph_info" / (n + ".hipdb")))
        assert np.array_equal(img.node_len, g.node_len) and np.array_equal(img.path_off, g.path_off) and np.array_equal(img.path_nodes, g.path_nodes)
        assert img.names == list(g.hap_names) and img.L == int(np.sum(g.node_len))
        assert np.array_equal(img.widths, codec.minimal_widths(g.path_nodes)) and img.len16 == (int(np.max(g.node_len)) < 65536)


def test_mixed_upload_through_the_file_seam(eng, world):
    """Images of every other species removed: packed species and species streamed from their .bin files meet in one db_upload_arrays (holes in the
    plain pipelines beside plain stretches).  The tables are the oracle's, and the bytes of the run without images."""
    for keep_parity in (0, 1):
        db2 = _copy_db(world, "db_mixed%d" % keep_parity)
        gone = [n for k, n in enumerate(world["images"]) if k % 2 != keep_parity]
        assert gone and len(gone) < len(world["images"])
        for n in gone:
            os.remove(db2 / "species_graph_info" / (n + ".hipdb"))
        wd = _run(eng, world, "wd_mixed%d" % keep_parity, db2, image_cache=1)
        _same_tables(wd, world["root"] / "wd_plain")
        assert not any((db2 / "species_graph_info" / (n + ".hipdb")).exists() for n in gone)      # image_cache 1 writes none


@pytest.mark.parametrize("case", ["A", "B"])
def test_file_seam_falls_back_from_a_damaged_offset_table(eng, world, case, capfd):
    """A stale or damaged image ends in the graph file, not in a failed run and not in a read outside the species' payload.
    A: the image of a species that is NOT the last of its load (one group: the set is small) is written with its last two blocks 2 and 1 bytes wide, and
    the entry between them is moved to one unit behind the species' payload.  The second-to-last block is then 4 bytes wide -- a width the old test
    accepts -- and ends one unit inside the next species' payload; the table's ends are consistent.  Only the device guard refuses that block (the last
    one has width -1 either way); the walk check reports it and the seam loads the graph files instead.  B: the last entry alone (width 0: never
    read) -- the header pass refuses the image.  Either way the tables are the oracle's and the bytes of the run without images."""
    db2 = _copy_db(world, "db_guard" + case)
    names = world["images"]
    by_name = {g.name: g for g in world["sset"].species}
    units = [codec.read_image(str(db2 / "species_graph_info" / (n + ".hipdb"))).payload_bytes // codec.UNIT for n in names]
    # never the last one loaded: the two units behind the victim's payload belong to the species loaded after it
    k = next(i for i in range(len(names) - 1) if units[i] >= 2 and sum(units[i + 1:]) >= 2)
    victim = names[k]
    p = str(db2 / "species_graph_info" / (victim + ".hipdb"))
    img = codec.read_image(p)
    widths = img.widths.copy()
    if case == "A":
        assert k < len(names) - 1 and widths[-2:].tolist() == [1, 1]                               # (walks along the backbone: one byte per step)
        widths[-2] = 2                                                                             # valid, not canonical
        off = np.concatenate([[0], np.cumsum(widths)]).astype(np.uint32)
        off[-2] = off[-1] + 1
        assert np.diff(off.astype(np.int64)).tolist()[-2:] == [4, -1] and int(off[-2]) - int(off[-1]) <= sum(units[k + 1:])
    else:
        off = img.blk_off.copy()
        off[-1] = off[-2]
    g = by_name[victim]
    st = os.stat(p)
    codec.write_image(p, g.node_len, g.path_off, g.path_nodes, list(g.hap_names), int(np.sum(g.node_len)), widths=widths, blk_off=off)
    os.utime(p, ns=(st.st_atime_ns, st.st_mtime_ns))
    capfd.readouterr()
    wd = _run(eng, world, "wd_guard" + case, db2, image_cache=1)
    err = capfd.readouterr().err
    _same_tables(wd, world["root"] / "wd_plain")
    # A: the load was tried, refused on the device and said so once, naming the image; B: the header pass dropped the image like a truncated one
    assert (("failed its load-time checks" in err and victim + ".hipdb" in err and "walks a node outside its species graph" in err) if case == "A"
            else "load-time checks" not in err), err
    wd = _run(eng, world, "wd_guard_rewrite" + case, db2, image_cache=2)                           # parsed again: the image is written afresh
    _same_tables(wd, world["root"] / "wd_plain")
    assert codec.read_image(p).same_graph(img)
