"""Which route a build of the unique-trio index takes (trio_plan / trio_index_build), pinned by the library's timer labels: every case uploads a db of
graphs alone, takes the stage call (pantax_hip_trio_index, then the tables), compares the four tables with the oracle's species by species, bit for bit,
and then asserts WHICH of the thirteen brackets of the build ran and which did not.  A rebuild case resets the timers behind the first build, so that
only the rebuild's labels are seen; the tables of every build are compared."""
import numpy as np
import pytest

VISIT, BLOCK, FILE = "trio_visit_kernel", "trio_block_kernel", "trio_file_kernel"
COUNT, FILL, UNIQ = "trio_count_kernel", "trio_fill_kernel", "trio_uniq_kernel"
PREFIX, SCAN_GROUP = "group_tile_prefix_kernel", "scan_chained_kernel<GroupCount>"
SCAN_SLOW, SCAN_FIRST = "scan_chained_kernel<SlowFirst>", "scan_chained_kernel<TrioFirst>"
ROWS, LOOKUP, CANON = "trio_rows_kernel", "trio_lookup_kernel", "trio_canon_kernel"
LABELS = {VISIT, BLOCK, FILE, COUNT, FILL, UNIQ, PREFIX, SCAN_GROUP, SCAN_SLOW, SCAN_FIRST, ROWS, LOOKUP, CANON}

# (haplotypes, genome length) per species, made one after the other from one generator (seed 20261020): `mixed` begins with narrow's first two species.
# narrow: no node is an interior position of more than 64 walks (the visit table takes every species); mixed: the species of 70 haplotypes has one
# (that species is the node-block kernel's).  A few thousand nodes each: the smallest shapes at which every route is still taken.
SEED = 20261020
SETS = {"narrow": [(1, 10000), (3, 20000), (6, 30000), (12, 15000)],
        "mixed": [(1, 10000), (3, 20000), (70, 12000)]}

# id, set, library options (set before the upload: trio_path=block is read there), rebuild (db_reset + a second stage call, whose labels are the ones
# asserted), the labels of LABELS that appear -- all others of LABELS must not
CASES = [
    ("first", "narrow", {}, False, {VISIT, PREFIX, ROWS}),
    ("rebuild", "narrow", {}, True, {FILE}),
    ("two_pass", "narrow", {"trio_two_pass": "1"}, True, {VISIT, PREFIX, ROWS}),
    ("prefix_chained", "narrow", {"flag_rank_chained": "1"}, False, {VISIT, SCAN_GROUP, ROWS}),
    ("rows_path", "narrow", {"trio_rows": "path"}, False, {VISIT, SCAN_FIRST, LOOKUP, CANON}),
    ("block", "narrow", {"trio_path": "block"}, False, {BLOCK, SCAN_FIRST, LOOKUP, CANON}),
    ("bucket", "narrow", {"trio_path": "bucket"}, False, {COUNT, FILL, UNIQ, SCAN_FIRST, LOOKUP, CANON}),
    ("mixed_first", "mixed", {}, False, {VISIT, BLOCK, PREFIX, ROWS, SCAN_SLOW, LOOKUP, CANON}),
    ("mixed_rebuild", "mixed", {}, True, {FILE, BLOCK, SCAN_SLOW, LOOKUP, CANON}),
]
# the three fused scans of the build (GroupCount, TrioFirst, SlowFirst) again under the 8192- and the 16384-item tile, which the size rule takes only from
# 2^22 / 2^26 items on (option scan_tile, scan_chained.hpp): same routes, same tables
CASES += [("%s_scan_%s" % (name, tile), key, dict(options, scan_tile=tile), rebuild, expected)
          for tile in ("big", "huge") for name, key, options, rebuild, expected in CASES if name in ("prefix_chained", "rows_path", "mixed_first")]


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def world():
    """set key -> (the graphs, the oracle's trio table of every species): made once, shared by the cases, never changed"""
    import synthdata as synth
    made = {}

    def get(key, with_oracle=True):
        if key not in made:
            rng = np.random.default_rng(SEED)
            species, start = [], 1
            for s, (h, gl) in enumerate(SETS[key]):
                g = synth.make_species(rng, str(1000 + s), h, gl, start, "GCF_%06d" % (s + 1))
                species.append(g)
                start = g.range_end + 1
            made[key] = [species, None]
        if with_oracle and made[key][1] is None:
            from oracle import oracle as orc
            made[key][1] = [orc.TrioTable(orc.Graph(g.node_len, g.path_off, g.path_nodes)) for g in made[key][0]]
        return made[key]
    return get


def _max_interior_visits(g):
    """the most walks' interior positions (every position but the first and the last of its walk) any node of the species is"""
    po = g.path_off.astype(np.int64)
    interior = np.ones(len(g.path_nodes), dtype=bool)
    interior[po[:-1][np.diff(po) > 0]] = False
    interior[(po[1:] - 1)[np.diff(po) > 0]] = False
    return int(np.bincount(g.path_nodes[interior]).max()) if interior.any() else 0


def test_the_sets_are_what_the_cases_need(world):
    narrow, _ = world("narrow", with_oracle=False)
    mixed, _ = world("mixed", with_oracle=False)
    assert [g.n_paths for g in narrow] == [1, 3, 6, 12] and [g.n_paths for g in mixed] == [1, 3, 70]
    assert all(_max_interior_visits(g) <= 64 for g in narrow)
    assert [_max_interior_visits(g) > 64 for g in mixed] == [False, False, True]
    for a, b in zip(narrow[:2], mixed[:2]):
        assert np.array_equal(a.path_nodes, b.path_nodes) and np.array_equal(a.node_len, b.node_len) and a.range_start == b.range_start
    assert all(sum(g.n_nodes for g in sset) < 8000 for sset in (narrow, mixed))
    assert all(len(g.path_nodes) >= 3 * g.n_paths for sset in (narrow, mixed) for g in sset)      # every walk has a window


def _timed_index(eng):
    """the stage call under the library's timers -> (abc, hap, len, hap_trio_off, the labels that ran)"""
    eng.timing_enable(True)
    eng.timing_reset()
    try:
        tables = eng.trio_nodes_info()
        ran = set(eng.timing_get())
    finally:
        eng.timing_enable(False)
    return tables, ran


def _check_against_oracle(eng, ref, tables):
    abc, hap, ln, hto = tables
    for si, T in enumerate(ref):
        h0, h1 = int(eng.hap_off[si]), int(eng.hap_off[si + 1])
        u0, u1 = int(hto[h0]), int(hto[h1])
        assert u1 - u0 == T.n_unique
        assert np.array_equal(abc[u0:u1], T.abc) and np.array_equal(hap[u0:u1], T.hap)
        assert np.array_equal(ln[u0:u1], T.len)
        assert np.array_equal(hto[h0:h1 + 1] - hto[h0], T.hap_off)
    assert int(hto[-1]) == eng.U == sum(T.n_unique for T in ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name,key,options,rebuild,expected", CASES, ids=[c[0] for c in CASES])
def test_route_and_tables(eng, world, set_opt, name, key, options, rebuild, expected):
    species, ref = world(key)
    assert sum(T.n_unique for T in ref) > 100
    for opt, value in options.items():
        set_opt(eng, opt, value)
    eng.upload_db(species)
    tables, ran = _timed_index(eng)
    _check_against_oracle(eng, ref, tables)
    if rebuild:
        print("%s, first build: %s" % (name, sorted(ran & LABELS)))
        eng.db_reset()
        tables, ran = _timed_index(eng)
        _check_against_oracle(eng, ref, tables)
    print("%s: %s" % (name, sorted(ran & LABELS)))
    assert ran & LABELS == expected, sorted(ran & LABELS)
