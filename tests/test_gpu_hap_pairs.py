"""GPU tests of the pairwise strain distinguishability of a db (pantax_hip_db_hap_pairs, the --db-pairs mode).  The expected values come from the numpy
restatement of the contract in tests/hap_pairs_ref.py (pinned by tests/test_hap_pairs_ref.py on a hand-computed case).  Everything is an integer: every
comparison is np.array_equal.  Each case runs under the default membership route and under hap_pairs_route=walk, and under the default chunk of the node
pass and under a small one (option hap_pairs_chunk), which puts chunk borders -- and so several flushes into the same counters -- inside small species."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines
from tests.hap_pairs_ref import HEADER, derived, hap_pairs, table

pytestmark = pytest.mark.gpu

CHUNK_MIN = 1024       # the node pass cuts a species' nodes into chunks of max(1024, 32 ka kb) nodes per block pair (hap_pairs_plan.hpp), taken 64 at a time
E_INVALID, E_LIMIT = -1, -4


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _selection(species, pick):
    off, hp = [0], []
    for s, g in enumerate(species):
        hp += list(pick(s, g.n_paths))
        off.append(len(hp))
    return np.array(off, dtype=np.uint64), np.array(hp, dtype=np.uint32)


def _check(got, exp):
    assert len(got) == len(exp) == 3
    for a, b in zip(got, exp):
        assert a.dtype == b.dtype == np.uint64 and a.shape == b.shape and np.array_equal(a, b)


def _all_ways(eng, set_opt, sel, small_chunk=128):
    """the call under the default route and under hap_pairs_route=walk, each with the default chunk and with a small one: the same numbers four times"""
    got = eng.hap_pairs(*sel)
    for route, chunk in ((None, small_chunk), ("walk", None), ("walk", small_chunk)):
        set_opt(eng, "hap_pairs_route", route)
        set_opt(eng, "hap_pairs_chunk", chunk)
        try:
            _check(eng.hap_pairs(*sel), got)
        finally:
            set_opt(eng, "hap_pairs_route", None)
            set_opt(eng, "hap_pairs_chunk", None)
    return got


def _block(res, s):
    """the K x K x 2 block of species s of a (pair_off, pair, species) result"""
    lo, hi = int(res[0][s]), int(res[0][s + 1])
    K = int(round((hi - lo) ** 0.5))
    assert K * K == hi - lo
    return res[1][lo:hi].reshape(K, K, 2)


def _identities(res):
    for s in range(len(res[2])):
        P, sp = _block(res, s), res[2][s]
        d = np.einsum("iiq->iq", P)
        assert np.array_equal(P, P.transpose(1, 0, 2))
        assert np.all(P <= np.minimum(d[:, None], d[None, :])) and (len(P) == 0 or np.all(sp[2] <= P))
        if len(P) == 1:
            assert np.array_equal(P[0, 0], sp[2])
        assert np.all(sp[1] + sp[2] <= sp[0])


def _mixed_species(seed, haps, genome_len):
    """species with a haplotype count of their own each (the graphs of the evidence tests' _mixed_set: the same generator calls in the same order)"""
    import synthdata as synth
    rng = np.random.default_rng(seed)
    species, start = [], 1
    for s, h in enumerate(haps):
        g = synth.make_species(rng, str(1000 + s), h, genome_len, start, "GCF_%06d" % (s + 1), present_frac=0.3)
        species.append(g)
        start = g.range_end + 1
    return species


@pytest.fixture(scope="module")
def narrow():
    import synthdata as synth
    return synth.make_set(921, 3, 6, 20000, 30000, present_frac=0.6)


def test_hap_pairs_narrow_routes_and_selections(eng, narrow, set_opt):
    """all haplotypes of one species, a shuffled three of the next, none of the last; by the node -> haplotype words and by the walks"""
    species = narrow.species
    eng.upload_db(species)                                                   # an uploaded db and nothing else: no reads, no coverage pass
    sel = _selection(species, lambda s, H: range(H) if s == 0 else ([] if s == 2 else [4, 0, 2]))
    exp = hap_pairs(species, *sel)
    # the case holds what the kernel can get wrong (computed from the set: a changed generator cannot hollow the test out)
    V = [g.n_nodes for g in species]
    assert all(g.n_paths == 6 for g in species)                              # <= 64 haplotypes: the default route is the node -> haplotype words
    assert V[0] > max(CHUNK_MIN, 32 * 6 * 6) and V[1] > max(CHUNK_MIN, 32 * 3 * 3)   # a chunk border inside both species under the default chunk
    assert all(v % 64 and (v % CHUNK_MIN) % 64 and (v % 128) % 64 for v in V[:2])    # a last tile that ends inside a wave
    assert exp[0].tolist() == [0, 36, 45, 45]
    for s in (0, 1):
        P, core = _block(exp, s), exp[2][s, 2]
        K = len(P)
        off = P[~np.eye(K, dtype=bool)]
        lo = np.minimum(np.einsum("iiq->iq", P)[:, None], np.einsum("iiq->iq", P)[None, :])[~np.eye(K, dtype=bool)]
        assert np.all(off > core) and np.all(off < lo)                       # off-diagonal entries strictly between core and the diagonal
    assert np.all(exp[2][:2, 2, 0] > 0) and exp[2][1, 1, 0] > 0              # core nodes; nodes none of the three walks
    assert np.array_equal(exp[2][2, 1], exp[2][2, 0]) and not exp[2][2, 2].any()     # nothing selected: every node is `none`, no core
    got = _all_ways(eng, set_opt, sel)
    _check(got, exp)
    _identities(got)
    assert eng.hap_pairs(*sel, species=False)[2] is None and np.array_equal(eng.hap_pairs(*sel, species=False)[1], exp[1])
    # one haplotype a species: pair = core
    one = _selection(species, lambda s, H: [s + 1])
    got1 = _all_ways(eng, set_opt, one)
    _check(got1, hap_pairs(species, *one))
    _identities(got1)
    assert all(np.array_equal(_block(got1, s)[0, 0], got1[2][s, 2]) for s in range(3))


def test_hap_pairs_64_and_65_haplotypes(eng, set_opt):
    """bit 63 of the one-word route (haplotype 63 of 64), and the first species with two words (65 haplotypes), where block pair (0, 1) has one live column"""
    species = _mixed_species(922, [64, 65], 8000)
    assert [g.n_paths for g in species] == [64, 65] and all(g.n_nodes > 128 and g.n_nodes % 64 for g in species)
    eng.upload_db(species)
    full = _selection(species, lambda s, H: range(H))
    exp = hap_pairs(species, *full)
    assert exp[0].tolist() == [0, 64 * 64, 64 * 64 + 65 * 65]
    P0, P1 = _block(exp, 0), _block(exp, 1)
    assert P0[63, 63, 0] > 0 and np.all(P0[63, :63, 0] > 0)                  # the last bit of the word, against every other
    assert P1[64, 64, 0] > 0 and np.all(P1[:64, 64, 0] > 0) and np.any(P1[:64, 64] != P1[64, 64])   # the one column of word 1, against every row of word 0
    got = _all_ways(eng, set_opt, full, small_chunk=64)
    _check(got, exp)
    _identities(got)
    part = _selection(species, lambda s, H: [63, 5, 20] if s == 0 else [64, 0, 33])   # a few bits of the word; the wide species through compact masks
    _check(_all_ways(eng, set_opt, part), hap_pairs(species, *part))


def test_hap_pairs_wide_species(eng, set_opt):
    """130 haplotypes, all selected in shuffled order: three words, six block pairs, the off-diagonal ones mirrored into the lower triangle"""
    species = _mixed_species(923, [130], 8000)
    assert species[0].n_paths == 130
    order = [int(h) for h in np.random.default_rng(7).permutation(130)]
    sel = _selection(species, lambda s, H: order)
    exp = hap_pairs(species, *sel)
    P = _block(exp, 0)
    d = np.einsum("iiq->iq", P)
    for a, b in ((3, 100), (70, 129), (0, 128), (129, 5), (100, 63)):        # members in different words, both ways round
        assert a // 64 != b // 64 and P[a, b, 0] > 0 and not np.array_equal(P[a, b], d[a]) and not np.array_equal(P[a, b], d[b])
    eng.upload_db(species)
    got = _all_ways(eng, set_opt, sel, small_chunk=64)
    _check(got, exp)
    _identities(got)
    part = _selection(species, lambda s, H: order[:70])                      # two words, six live columns in the second
    _check(_all_ways(eng, set_opt, part), hap_pairs(species, *part))


def test_hap_pairs_identical_and_nested(eng, narrow, set_opt):
    """a haplotype whose walk is another's in a different order with a node repeated: identical; one whose walk is a strict subset of another's: nested"""
    g = narrow.species[0]
    walks = [g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])] for h in range(g.n_paths)]
    twin = np.concatenate([walks[2][::-1], walks[2][:1]])                    # hap 2 backwards, its first node once more
    part = walks[0][::2]                                                     # every other step of hap 0
    assert len(set(part.tolist())) < len(set(walks[0].tolist()))
    walks += [twin, part]
    off = np.concatenate([[0], np.cumsum([len(w) for w in walks])]).astype(np.uint64)
    g2 = dataclasses.replace(g, path_off=off, path_nodes=np.concatenate(walks).astype(np.uint32), hap_names=g.hap_names + ["zz_twin", "zz_part"],
                             genome_len=np.concatenate([g.genome_len, g.genome_len[:2]]), truth_depth=np.concatenate([g.truth_depth, g.truth_depth[:2]]))
    assert g2.n_paths == 8
    eng.upload_db([g2])
    sel = _selection([g2], lambda s, H: range(H))
    got = _all_ways(eng, set_opt, sel)
    _check(got, hap_pairs([g2], *sel))
    P = _block(got, 0)
    assert derived(P, 2, 6)[2:4] == (0, "identical") and np.array_equal(P[2, 2], P[2, 6]) and np.array_equal(P[6, 6], P[2, 6])
    only_a, only_b, dist, cls, _ = derived(P, 0, 7)
    assert cls == "nested" and only_a > 0 and only_b == 0 and dist == only_a and np.array_equal(P[7, 7], P[0, 7])
    assert derived(P, 0, 1)[3] == "distinct"


def _raw(eng, sel_off, sel_hap, cap, n_species=None, fill=77):
    """the C call as it is: (rc, pair_off, pair, species); the arrays are pre-filled with `fill`"""
    from pantax_amd import _ffi
    so, sh = np.ascontiguousarray(sel_off, dtype=np.uint64), np.ascontiguousarray(sel_hap, dtype=np.uint32)
    cs = _ffi.EvidenceSet(eng.S if n_species is None else n_species, so.ctypes.data, sh.ctypes.data if len(sh) else None)
    pair_off = np.full(eng.S + 1, fill, dtype=np.uint64)
    pair = np.full((max(cap, 1), 2), fill, dtype=np.uint64)
    sp = np.full((eng.S, 3, 2), fill, dtype=np.uint64)
    rc = eng.lib.pantax_hip_db_hap_pairs(eng.ctx, eng.db, C.byref(cs), _ffi.p(pair_off), cap, _ffi.p(pair), _ffi.p(sp))
    return rc, pair_off, pair, sp


def test_hap_pairs_sizing_and_arguments(eng, narrow):
    species = narrow.species
    eng.upload_db(species)
    sel = _selection(species, lambda s, H: [4, 1] if s == 1 else ([H - 1] if s == 0 else []))
    exp = hap_pairs(species, *sel)
    # pair_cap = 0 sizes the output; one entry short is still short
    for cap in (0, 4):
        rc, pair_off, pair, sp = _raw(eng, *sel, cap)
        assert rc == E_LIMIT and pair_off.tolist() == [0, 1, 5, 5] and np.all(pair == 77) and np.all(sp == 77)
    rc, pair_off, pair, sp = _raw(eng, *sel, 5)
    assert rc == 0
    _check((pair_off, pair, sp), exp)
    # refused arguments: nothing is written
    for args, kw in ((([0, 0, 2, 2], [3, 3]), {}),                           # a haplotype twice within a species
                     (([0, 1, 1, 1], [species[0].n_paths]), {}),             # index = n_paths
                     ((sel[0][:-1], sel[1]), {"n_species": eng.S - 1})):
        rc, pair_off, pair, sp = _raw(eng, *args, 64, **kw)
        assert rc == E_INVALID and np.all(pair == 77) and np.all(sp == 77)
    # nothing selected: no entry, every node of every species is `none`
    rc, pair_off, pair, sp = _raw(eng, [0, 0, 0, 0], [], 0)
    assert rc == 0 and not pair_off.any() and np.all(pair == 77) and np.array_equal(sp[:, 0], sp[:, 1]) and not sp[:, 2].any()
    assert sp[:, 0, 0].tolist() == [g.n_nodes for g in species] and np.array_equal(sp[:, 0], exp[2][:, 0])


def test_hap_pairs_256_served_257_refused(eng, set_opt):
    from pantax_amd._ffi import PantaxHipError
    species = _mixed_species(925, [257, 3], 3000)
    assert species[0].n_paths == 257
    eng.upload_db(species)
    wide = _selection(species, lambda s, H: range(H))
    rc, pair_off, pair, sp = _raw(eng, *wide, 257 * 257 + 9)
    assert rc == E_LIMIT and np.all(pair == 77) and np.all(sp == 77)
    with pytest.raises(PantaxHipError) as e:
        eng.hap_pairs(*wide)
    assert e.value.code == E_LIMIT and "species 0" in str(e.value) and "257" in str(e.value)
    most = _selection(species, lambda s, H: range(1, H) if s == 0 else [2])  # 256 of them: four full words, ten block pairs
    exp = hap_pairs(species, *most)
    assert exp[0].tolist() == [0, 65536, 65537]
    got = eng.hap_pairs(*most)
    _check(got, exp)
    _identities(got)
    set_opt(eng, "hap_pairs_chunk", 64)
    _check(eng.hap_pairs(*most), exp)


def test_hap_pairs_stateless_and_ties_to_evidence(eng, narrow):
    """on a set with a coverage result the call changes nothing the evidence call reads, and its sums are the evidence call's in the columns they share"""
    sset = narrow
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    eng.get_node_abundances(fetch=False)
    sel = _selection(sset.species, lambda s, H: [5, 1, 3] if s == 1 else ([3, 0] if s == 0 else []))
    before = eng.strain_evidence(*sel)
    got = eng.hap_pairs(*sel)
    after = eng.strain_evidence(*sel)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    hap, sp = before
    assert hap[:, 0, 2].sum() > 0 and sp[:, 0, 3].sum() > 0                  # the evidence call did see coverage
    diag = np.concatenate([np.einsum("iiq->iq", _block(got, s)) for s in range(3)])
    assert np.array_equal(diag, hap[:, 0, :2])                               # the diagonal = {n_nodes, len} of `all`
    assert np.array_equal(got[2], sp[:, :, :2])                              # total, none, core = total, orphan, core
    _check(got, hap_pairs(sset.species, *sel))
    eng.profile_step(sset.avg_len())                                         # behind a resident step too (the evidence call is refused there)
    _check(eng.hap_pairs(*sel), hap_pairs(sset.species, *sel))


# ---- the --db-pairs mode ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """a db directory of four species of 5, 1, 5, 1 haplotypes; species 0 gets a twin of its haplotype 1 (an identical pair) and a part of its haplotype 0"""
    import synthdata as synth
    from pantax_amd.engine import Engine
    sset = synth.make_set(926, 4, 5, 200, 12000, present_frac=0.5, single_strain_every=2)
    g = sset.species[0]
    walks = [g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])] for h in range(g.n_paths)]
    walks += [np.concatenate([walks[1][::-1], walks[1][:1]]), walks[0][::2]]
    off = np.concatenate([[0], np.cumsum([len(w) for w in walks])]).astype(np.uint64)
    last = g.hap_names[-1]
    names = g.hap_names + [last[:-5] + "998.1", last[:-5] + "999.1"]
    assert names == sorted(names) and len(set(names)) == 7
    sset.species[0] = dataclasses.replace(g, path_off=off, path_nodes=np.concatenate(walks).astype(np.uint32), hap_names=names,
                                          genome_len=np.concatenate([g.genome_len, g.genome_len[:2]]), truth_depth=np.concatenate([g.truth_depth, g.truth_depth[:2]]))
    root = tmp_path_factory.mktemp("pantax_db_pairs")
    db = root / "db"
    db.mkdir()
    synth.write_db(sset, str(db))
    e = Engine(0)
    yield sset, root, db, e
    e.close()


def _genome_id(g, h):
    return "%s_ASM%sv1" % (g.hap_names[h], g.hap_names[h][4:10])             # synthdata.write_db's genomes_info.txt


def _same_table(path, exp):
    rows = _lines(path)
    assert len(rows) == len(exp) and rows[0] == exp[0] == HEADER
    for r, x in zip(rows[1:], exp[1:]):
        assert r[:13] == x[:13]
        assert r[13] == "-" if isinstance(x[13], str) else np.float64(r[13]) == x[13]


def test_db_pairs_cli(world, set_opt):
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, eng = world
    species = sset.species
    assert [g.n_paths for g in species] == [7, 1, 5, 1]
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")

    def cli(out, *extra):
        return subprocess.run([exe, "-db", str(db), "--db-pairs", str(out)] + [str(x) for x in extra], cwd=str(root), capture_output=True, text=True, timeout=120)

    # the default: every species with more than one haplotype, in range-file order
    r = cli(root / "all.tsv")
    assert r.returncode == 0, r.stderr
    exp = table([species[0], species[2]], _genome_id)
    classes = [x[3] for x in exp[1:]]
    assert classes.count("identical") == 1 and classes.count("nested") >= 1 and classes.count("distinct") >= 10 and classes[-2:] == ["species", "species"]
    assert len(exp) == 1 + 21 + 10 + 2 and exp[-2][12] == "0" and int(exp[-1][12]) > 0
    _same_table(root / "all.tsv", exp)
    # the library call writes the same bytes; so do the GFA loader and a db that goes through the device species by species
    eng.db_pairs(db, root / "lib.tsv")
    eng.db_pairs(db, root / "gfa.tsv", zip=None)
    set_opt(eng, "db_path_steps_max", 1)
    eng.db_pairs(db, root / "groups.tsv")
    set_opt(eng, "db_path_steps_max", None)
    for f in ("lib.tsv", "gfa.tsv", "groups.tsv"):
        assert open(root / f, "rb").read() == open(root / "all.tsv", "rb").read()
    r = cli(root / "gfa_cli.tsv", "--gfa")
    assert r.returncode == 0 and open(root / "gfa_cli.tsv", "rb").read() == open(root / "all.tsv", "rb").read()
    # one named species; a single-haplotype species has a species row alone, without a distance
    r = cli(root / "one.tsv", "--db-pairs-species", species[2].name)
    assert r.returncode == 0, r.stderr
    _same_table(root / "one.tsv", table([species[2]], _genome_id))
    r = cli(root / "two.tsv", "--db-pairs-species", "%s,%s" % (species[2].name, species[1].name))
    assert r.returncode == 0, r.stderr
    exp2 = table([species[1], species[2]], _genome_id)                      # range-file order, not the option's
    assert exp2[-2][:4] == [species[1].name, "1", "-", "species"] and exp2[-2][12] == "-"
    _same_table(root / "two.tsv", exp2)
    # identical pairs only: the species rows keep the smallest distance over all pairs
    r = cli(root / "zero.tsv", "--db-pairs-max-distance", 0)
    assert r.returncode == 0, r.stderr
    exp0 = table([species[0], species[2]], _genome_id, max_distance=0)
    assert [x[3] for x in exp0[1:]] == ["identical", "species", "species"] and exp0[1][1:3] == [_genome_id(species[0], 1), _genome_id(species[0], 5)]
    _same_table(root / "zero.tsv", exp0)
    # an unknown taxid: refused, nothing written
    r = cli(root / "unknown.tsv", "--db-pairs-species", species[0].name + ",424242")
    assert r.returncode != 0 and "424242" in r.stderr and not os.path.exists(root / "unknown.tsv")
    with pytest.raises(PantaxHipError) as e:
        eng.db_pairs(db, root / "unknown.tsv", species=["424242"])
    assert e.value.code == E_INVALID
