"""The text the seven read passes share (read_pass_device.hpp: the species rounds of a wave, the lane-per-slot prologue of the long-walk kernels, the
one-word membership), pinned by running all seven calls -- read_strains, strain_read_support, strain_read_em, strain_mosaic, strain_read_rescue,
strain_links, strain_rarefy -- on ONE small set, each against the reference its own test file uses, on both membership routes, exactly.

Why the set is so small.  The upload-time layout (stage_read_layout.hip) buckets reads by `first node id >> (5 + g)`, and g grows until a unit holds
about 2048 steps.  The five species here have 8 .. 12 nodes each with consecutive node ids (50 ids in all) and the reads hold about 1600 steps, so every
read shares one unit; slot order inside a unit is arbitrary, the species are interleaved in file order, and a 64-step group of one- to three-step reads
therefore holds deciding lanes of three or more species.  The larger sets of the calls' own tests keep a species' reads together and give "one or two
rounds" of the species loop; this set is the one that gives three or more.  The walks of exactly 64, 65 and 130 steps (two species) go through the
lane-per-slot kernels, a walk of 64 ends on lane 63; a read binned to no species and an empty walk own no deciding lane.

The species: two with three chosen strains, one with none chosen (route 0: counted only), one of 65 haplotypes with all of them chosen (two mask words:
handed to read_strains and strain_read_support, whose contract serves more than 64 candidates; the other calls get 64 of its 65), one of 64 haplotypes
with exactly 64 chosen (bit 63)."""
import numpy as np
import pytest

from tests import links_ref, mosaic_ref, rarefy_ref, rescue_ref
from tests.read_em_ref import read_classes, species_estimates
from tests.test_gpu_mosaic import _hap_nodes, _rows
from tests.test_gpu_read_strains import _expected as read_strains_expected
from tests.test_gpu_read_support import _reference as read_support_reference

pytestmark = pytest.mark.gpu

SEED = 20261021
N_NODES = (10, 8, 12, 11, 9)
N_HAPS = (4, 3, 65, 64, 5)
WIDE, FULL = 2, 3                       # the 65-haplotype species, the species with exactly 64 chosen
LONG = (64, 65, 130)
RAREFY = dict(seed=42, n_levels=3, n_replicates=2)
EM_ITER, EM_TOL = 7, 1e-6
u64, u32 = lambda x: np.array(x, dtype=np.uint64), lambda x: np.array(x, dtype=np.uint32)


def _build():
    import synthdata as synth
    rng = np.random.default_rng(SEED)
    species, start = [], 1
    for s, (V, H) in enumerate(zip(N_NODES, N_HAPS)):
        walks = []
        for h in range(H):
            keep = np.nonzero((rng.random(V) < 0.7) | (np.arange(V) < 2))[0]      # nodes 0 and 1 are core: a read of them fits every strain
            walks.append(keep.astype(np.uint32))
        node_len = rng.integers(5, 41, size=V).astype(np.int64)
        off = np.concatenate([[0], np.cumsum([len(w) for w in walks])]).astype(np.uint64)
        species.append(synth.SpeciesGraph(str(3000 + s), node_len, off, np.concatenate(walks), ["GCF_9%02d%03d.1" % (s, h) for h in range(H)], start,
                                          start + V - 1, np.array([node_len[w].sum() for w in walks], dtype=np.int64), np.zeros(H)))
        start += V
    reads = []                          # (global node ids, pstart, pend)

    def add(s, local, ps=0, pe=None):
        local = np.asarray(local, dtype=np.int64)
        reads.append((local + species[s].range_start, ps, int(species[s].node_len[local].sum()) - 1 if pe is None else pe))

    def path(s, h):
        g = species[s]
        return g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])].astype(np.int64)
    longs = []
    for s in (0, FULL):                 # the walks of exactly 64, 65 and 130 steps: along one haplotype (it fits), and over every node (it fits nobody)
        for k in LONG:
            longs.append((s, np.resize(path(s, 1), k)))
            longs.append((s, np.resize(np.arange(N_NODES[s]), k)))
    for r in range(300):                # species interleaved in file order
        s = r % 5
        if r % 20 == 7 and longs:
            add(*longs.pop())
        k = 1 + int(rng.integers(0, 3))
        if rng.random() < 0.8:          # a stretch of a haplotype's walk
            p = path(s, int(rng.integers(0, N_HAPS[s])))
            at = int(rng.integers(0, len(p) - k + 1))
            add(s, p[at:at + k], ps=int(rng.integers(0, 3)))
        else:                           # any nodes of the species
            add(s, rng.integers(0, N_NODES[s], size=k), ps=int(rng.integers(0, 3)))
        if r == 150:
            reads.append((np.array([species[1].range_end, species[2].range_start], dtype=np.int64), 0, 9))   # binned to no species
            reads.append((np.zeros(0, dtype=np.int64), 0, 0))                                                  # an empty walk
            add(3, path(3, 5)[:2], ps=4, pe=1)                                                                 # pend < pstart: span 0
    assert not longs
    R = len(reads)
    packed = synth.PackedReads(np.concatenate([[0], np.cumsum([len(r[0]) for r in reads])]).astype(np.uint64),
                               np.concatenate([r[0] for r in reads]).astype(np.uint32), None, np.array([r[1] for r in reads], dtype=np.int64),
                               np.array([r[2] for r in reads], dtype=np.int64), np.full(R, 30000, dtype=np.int64), np.full(R, 60, dtype=np.int64),
                               np.full(R, 30000, dtype=np.int64))
    # what each species hands to the calls: chosen (file order, not sorted) and, for the rescue pass, unreported candidates
    chosen = [[2, 0, 3], [], [int(h) for h in rng.permutation(65)], [int(h) for h in rng.permutation(64)], [4, 1, 2]]
    narrow = [c if s != WIDE else [h for h in c if h != 17] for s, c in enumerate(chosen)]          # 64 of the 65
    sel = [[2, 0], [], narrow[WIDE][:34], narrow[FULL][:40], [4]]
    cand = [[3, 1], [1], narrow[WIDE][34:], narrow[FULL][40:], [1, 2, 0]]
    off = lambda lists: u64(np.cumsum([0] + [len(x) for x in lists]))
    flat = lambda lists: u32(sum(lists, []))
    weights = lambda lists: np.array([rng.choice([1.0, 2.5, 7.25]) for _ in sum(lists, [])], dtype=np.float64)
    sets = {"wide": (off(chosen), flat(chosen), weights(chosen)), "narrow": (off(narrow), flat(narrow), weights(narrow)),
            "rescue": (off(sel), flat(sel), off(cand), flat(cand))}
    return species, packed, sets


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.fixture(scope="module")
def world():
    """the engine with the set resident behind a coverage pass, and call -> the reference's numbers; made once, never changed"""
    from pantax_amd.engine import Engine
    species, reads, sets = _build()
    R = reads.n_reads
    flags = np.zeros(R, dtype=np.uint8)
    sp, rows = _rows(species, reads, flags)
    hap_nodes = _hap_nodes(species)
    k = np.diff(reads.step_off.astype(np.int64))
    assert 300 <= R <= 320 and all((k == n).sum() == 4 for n in LONG) and (k == 0).sum() == 1 and set(k.tolist()) <= {0, 1, 2, 3, *LONG}
    assert (sp < 0).sum() == 2 and all((sp == s).sum() >= 60 for s in range(5))          # no species: the straddling read and the empty walk
    assert {int(sp[r]) for r in np.nonzero(k > 63)[0]} == {0, FULL}
    assert len({int(s) for s in sp[100:105]}) == 5                                        # interleaved in file order
    eng = Engine(0)
    eng.upload_db(species)
    eng.upload_reads(reads.step_off, reads.node_id, reads.pstart, reads.pend, reads.qlen, reads.mapq, flags)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    bases = np.asarray(eng.get_node_abundances()[0]).astype(np.int64)
    node_off = np.cumsum([0] + list(N_NODES))
    per_species = [bases[node_off[s]:node_off[s + 1]] for s in range(5)]
    for s, g in enumerate(species):                                                       # the coverage pass the links and rarefy passes stand on
        assert np.array_equal(per_species[s], rarefy_ref.species_bases(g, reads, sp == s))
    wide, narrow, resc = sets["wide"], sets["narrow"], sets["rescue"]
    fill = (np.full(R, 12345, dtype=np.uint32), np.full(R, -7, dtype=np.int32), np.full(R, 0.5))
    lens = u64([int(species[s].genome_len[h]) for s in range(5) for h in narrow[1][int(narrow[0][s]):int(narrow[0][s + 1])]])
    classes = read_classes(hap_nodes, rows, narrow[0], narrow[1])
    walks = [[g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])].tolist() for h in range(g.n_paths)] for g in species]
    refs = {"read_strains": read_strains_expected(species, reads.step_off, reads.node_id, sp, np.ones(R, dtype=bool), *wide, fill),
            "read_support": read_support_reference(species, reads, flags, wide)[1],
            "read_em": tuple(classes) + tuple(species_estimates(narrow[0], narrow[1], lens, classes[1], classes[2], classes[3], EM_ITER, EM_TOL)),
            "mosaic": mosaic_ref.mosaic(hap_nodes, rows, *narrow),
            "rescue": rescue_ref.rescue(hap_nodes, rows, *resc),
            "links": links_ref.links(walks, [g.node_len for g in species], per_species, rows, narrow[0], narrow[1]),
            "rarefy": rarefy_ref.stage_reference(species, reads, sp, np.ones(R, dtype=bool), narrow[0], narrow[1], RAREFY["seed"], RAREFY["n_levels"],
                                                 RAREFY["n_replicates"])}
    yield eng, species, reads, sp, sets, fill, lens, refs
    eng.close()


def test_the_references_have_something_to_say(world):
    _, species, reads, sp, sets, _, _, refs = world
    hap, n, _ = refs["read_strains"]
    assert (n > 64).sum() > 0 and (n == 0).sum() > 0 and (n == -1).sum() >= 60 and (n == -7).sum() == 2   # two words; nothing fits; route 0; no species
    sup_hap, sup_species, pair_off, _ = refs["read_support"]
    assert (sup_species[:, 0, 0] >= 60).all() and not sup_species[1, 1:].any() and sup_species[[0, WIDE, FULL, 4], 1, 0].sum() > 0
    assert pair_off[WIDE + 1] == pair_off[WIDE] and pair_off[FULL + 1] - pair_off[FULL] == 64 * 64
    assert sup_hap[int(sets["wide"][0][FULL]):int(sets["wide"][0][FULL + 1]), 0, 0].min() > 0
    cls_off = refs["read_em"][1]
    assert all(cls_off[s + 1] - cls_off[s] >= 2 for s in (0, WIDE, FULL, 4)) and cls_off[2] == cls_off[1]
    mos_species = refs["mosaic"][0]
    assert mos_species[:, mosaic_ref.MOSAIC1:mosaic_ref.FOREIGN, 0].sum() > 0 and mos_species[:, mosaic_ref.FOREIGN, 0].sum() > 0 and refs["mosaic"][7] > 0
    res_species = refs["rescue"][0]
    assert res_species[:, rescue_ref.FOREIGN, 0].sum() > 0 and res_species[:, rescue_ref.MOSAIC, 0].sum() > 0 and refs["rescue"][2][:, 0, 0].sum() > 0
    lk_species = refs["links"][0]
    assert (lk_species[:, links_ref.CROSSINGS] > 0).all() and lk_species[:, links_ref.KNOWN].sum() > 0 and lk_species[:, links_ref.KNOWN + 1:].sum() > 0
    rf = refs["rarefy"]
    assert all(rf[0][s]["reads"][0] == (sp == s).sum() for s in (0, WIDE, FULL, 4)) and rf[0][1]["reads"] == [0, 0]
    assert any(0 < rec["reads"][0] < rf[0][s]["reads"][0] for per in rf[1:] for s, rec in enumerate(per))


def _same(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        if isinstance(e, np.ndarray):
            assert g.dtype == e.dtype and g.shape == e.shape
            assert np.array_equal(_bits(g), _bits(e))
        else:
            assert g == e


def _check_links(got, exp):
    species, table, hap, brk_off, rec = exp
    _same(got[:4], (species, table, hap, brk_off))
    step, start, node_a, node_b, flank, mask = got[4:]
    assert list(zip(step.tolist(), start.tolist(), node_a.tolist(), node_b.tolist(), flank.tolist(), mask.tolist())) == rec


def _check_rarefy(eng, got, sets, refs, species, reads, sp):
    x, obj, rows, status, n_reads, member = got
    off = sets["narrow"][0]
    for e, per in enumerate(refs["rarefy"]):
        for s, rec in enumerate(per):
            c0, c1 = int(off[s]), int(off[s + 1])
            assert rec["status"] != "limit"
            assert int(rows[e, s]) == rec["n_rows"] and int(status[e, s]) == rec["status"], (e, s)
            assert n_reads[e, s].tolist() == rec["reads"], (e, s, n_reads[e, s].tolist(), rec["reads"])
            assert np.array_equal(member[e, c0:c1], rec["member"]), (e, s)
    # the pass over the reads alone: the node bases of one level are the coverage pass's over the reads of the level
    for b, level in ((1, 0), (1, 1), (2, 2)):
        d = rarefy_ref.depths(RAREFY["seed"], b, reads.n_reads)
        exp = np.concatenate([rarefy_ref.species_bases(g, reads, (sp == s) & (d >= level)) for s, g in enumerate(species)]).astype(np.uint64)
        assert np.array_equal(eng.rarefy_node_bases(RAREFY["seed"], b, level), exp), (b, level)


CALLS = ("read_strains", "read_support", "read_em", "mosaic", "rescue", "links", "rarefy")


@pytest.mark.parametrize("route", ["default", "walk"])
@pytest.mark.parametrize("which", CALLS)
def test_call_equals_its_reference(world, set_opt, which, route):
    eng, species, reads, sp, sets, fill, lens, refs = world
    if route == "walk":
        set_opt(eng, "rarefy_route" if which == "rarefy" else "read_strain_route", "walk")
    wide, narrow, resc = sets["wide"], sets["narrow"], sets["rescue"]
    if which == "read_strains":
        _same(eng.read_strains(*wide, fill=tuple(np.array(a, copy=True) for a in fill)), refs[which])
    elif which == "read_support":
        _same(eng.strain_read_support(*wide), refs[which])
    elif which == "read_em":
        _same(eng.strain_read_em(narrow[0], narrow[1], lens, EM_ITER, EM_TOL), refs[which])
    elif which == "mosaic":
        _same(eng.strain_mosaic(*narrow), refs[which])
    elif which == "rescue":
        _same(eng.strain_read_rescue(*resc), refs[which])
    elif which == "links":
        _check_links(eng.strain_links(narrow[0], narrow[1]), refs[which])
    else:
        got = eng.strain_rarefy(narrow[0], narrow[1], **RAREFY)
        _check_rarefy(eng, got, sets, refs, species, reads, sp)
        if route == "walk":                                                              # x and obj: the same bits as on the default route
            set_opt(eng, "rarefy_route", None)
            for a, b in zip(got, eng.strain_rarefy(narrow[0], narrow[1], **RAREFY)):
                assert a.tobytes() == b.tobytes()
