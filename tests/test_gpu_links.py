"""GPU tests of the link support (pantax_hip_strain_links, --strain-links).  The expected integers come from the row-by-row reading of the contract in
tests/links_ref.py (pinned by hand in tests/test_links_ref.py); everything compares element for element.  The fixture is built node by node: its
aligned bases per node come from the rule of the coverage pass restated below (profile.rs:800-882 as oracle/pantax_oracle.c reads it), so that every
class the fixture is meant to hold is asserted on the CPU before any GPU call, and the device's coverage result is then compared against that rule."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import links_ref as ref
from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile, seam_world

pytestmark = pytest.mark.gpu

E_INVALID, E_LIMIT, E_STATE = -1, -4, -7
TILE = 1024                                                                  # CT_TILE: path positions per tile of the walk pass
u64, u32 = lambda x: np.array(x, dtype=np.uint64), lambda x: np.array(x, dtype=np.uint32)


def _graph(synth, i, node_len, walks, start):
    off = np.concatenate([[0], np.cumsum([len(w) for w in walks])]).astype(np.uint64)
    nodes = np.concatenate([np.asarray(w, dtype=np.uint32) for w in walks])
    names = ["GCF_7%02d%03d.1" % (i, h) for h in range(len(walks))]
    node_len = np.asarray(node_len, dtype=np.int64)
    return synth.SpeciesGraph(str(2000 + i), node_len, off, nodes, names, start, start + len(node_len) - 1,
                              np.array([node_len[np.asarray(w)].sum() for w in walks], dtype=np.int64), np.zeros(len(walks)))


def zig(a, b, n):
    return [a if i % 2 == 0 else b for i in range(n)]


def _build():
    """Nine species: four tiny ones (their reads share one 64-step group; species 3 has two strains on the same links: core), K_s = 0, the crafted
    species 5 (walks of 2049, 1024, 2, 1025, 18 and 1 steps in that list order, behind a filler walk that aligns them to the tiles), a 64-haplotype
    species with all of them selected (bit 63), a 70-haplotype species with 66 selected (skipped), and one that is left out of the db."""
    import synthdata as synth
    rng = np.random.default_rng(11)
    lens = lambda n: rng.integers(1, 41, size=n)
    walks = [
        [[0, 1, 2], [0, 2]],
        [[0, 1], [1, 2, 3]],
        [[0, 1, 2, 3], [3]],
        [[0, 1, 2], [2, 1, 0], [0, 2]],
        [[0, 1, 2, 3, 4]],
    ]
    sel = [[0], [1], [0], [1, 0], []]
    n_nodes = [3, 4, 4, 3, 5]
    before = sum(len(w) for ws in walks for w in ws)
    pad = (-before) % TILE or TILE
    hub = [2150 + (j + 1) // 2 if j % 2 else 2150 for j in range(18)]          # 2150 2151 2150 2152 .. 2150 2159: nine larger neighbours
    walks.append([
        [2190 + (i % 2) for i in range(pad)],                               # h0: the filler, not selected; its nodes are nobody's
        [0, 1, 0, 5, 5] + list(range(6, 6 + TILE - 5)),                     # h1: 1024 steps, u v u and u u; begins and ends at a tile border
        list(range(TILE)) + [2100],                                         # h2: 1025 steps: its last link lies on a tile border
        list(range(2 * TILE + 1)),                                          # h3: 2049 steps, begins at tile position 1: links on two borders
        [2195],                                                             # h4: one step
        [2196, 2197],                                                       # h5: two steps
        hub,                                                                # h6
    ])
    sel.append([3, 1, 5, 2, 6, 4])                                          # not in ascending order: bit p = position p
    n_nodes.append(2200)
    walks.append([[0, 1, 2, 3] + ([4 + j % 3] if j < 63 else [8, 9]) for j in range(64)])
    sel.append(list(range(64)))
    n_nodes.append(12)
    walks.append([[0, 1, 2] + ([3] if j % 2 else []) for j in range(70)])
    sel.append(rng.permutation(70)[:66].tolist())
    n_nodes.append(4)
    walks.append([[0, 1, 2]])                                               # left out of the db
    n_nodes.append(3)
    species, start = [], 1
    for i, (ws, n) in enumerate(zip(walks, n_nodes)):
        species.append(_graph(synth, i, lens(n), ws, start))
        start = species[-1].range_end + 1
    reads, marks = [], {}

    def add(s, nodes, name, pstart=0, flag=0):
        marks.setdefault(name, []).append(len(reads))
        ln = species[s].node_len
        reads.append((s, list(nodes), pstart, int(sum(int(ln[v]) for v in nodes)), flag))

    for s in (0, 1, 2, 3, 0, 1, 2, 3):
        add(s, [0, 1, 2], "tiny")
    for nodes in ([0, 1, 2, 3], [4], [2, 3]):
        add(4, nodes, "k0")
    add(5, [501, 500], "reverse")                                           # crosses {500, 501} against the walk order
    add(5, [500, 501, 502], "forward", pstart=1)
    add(5, [1021, 1022], "left_of_border")                                  # {1022, 1023}: both ends covered, never crossed -- h3's first tile border
    add(5, [1023, 1024], "right_of_border")                                 # ... and 1024 covered, 1025 not: {1024, 1025} stays open
    add(5, [2100], "single_2100")                                           # {1023, 2100}: h2's border link, private and broken
    add(5, [2045, 2046], "left_of_border2")
    add(5, [2047], "single_2047")                                           # 2047 is covered by single-step reads only: {2046, 2047} is broken on h3's second border
    add(5, [2047], "single_2047")
    add(5, [10, 20], "skip")
    add(5, [2100, 2155], "switch")                                          # h2 alone walks 2100, the hub alone 2155
    add(5, [5, 2190], "foreign")
    add(5, [2150, 2155], "hub")
    add(5, [2159, 2150], "hub")
    add(5, [0, 1, 0], "uvu")
    add(5, [5, 5], "uu")
    add(5, [2195], "one_step_walk")
    add(5, [2196, 2197], "two_step_walk")
    add(5, [10, 20], "dropped", flag=1)
    add(5, zig(10, 11, 63) + [20], "long64")                                # the only skip at steps 62|63
    add(5, zig(10, 11, 64) + [20], "long65")                                # ... at 63|64: the lane at a group's end looks into the next group
    add(5, zig(10, 11, 64) + zig(20, 21, 66), "long130_63")
    add(5, zig(10, 11, 65) + zig(20, 21, 65), "long130_64")
    add(5, zig(10, 11, 128) + zig(20, 21, 2), "long130_127")
    add(5, zig(30, 31, 130), "long130_known")
    for lo, hi in ((100, 900), (1100, 2000)):                               # sub-walks of h3 away from the hand-placed links
        for _ in range(150):
            a, k = int(rng.integers(lo, hi)), int(rng.integers(1, 7))
            add(5, range(a, a + k), "bulk", pstart=int(rng.integers(0, 2)) if species[5].node_len[a] > 1 else 0, flag=1 if rng.random() < 0.05 else 0)
    for nodes in ([0, 1, 2], [0, 1, 2], [2, 3], [8], [9], [8, 0], [3, 5], [3, 4], [1, 0]):
        add(6, nodes, "wide64")
    for nodes in ([0, 1, 2], [1, 2], [2, 3], [0]):
        add(7, nodes, "skipped")
    add(8, [0, 1], "not_in_db")
    add(8, [2], "not_in_db")
    db = species[:8]
    step_off = np.concatenate([[0], np.cumsum([len(r[1]) for r in reads])]).astype(np.uint64)
    node_id = np.concatenate([np.asarray(r[1], dtype=np.uint32) + np.uint32(species[r[0]].range_start) for r in reads])
    R = len(reads)
    arrays = dict(step_off=step_off, node_id=node_id, pstart=np.array([r[2] for r in reads], dtype=np.int64), pend=np.array([r[3] for r in reads], dtype=np.int64),
                  qlen=np.full(R, 30000, dtype=np.int64), mapq=np.full(R, 60, dtype=np.int64), flags=np.array([r[4] for r in reads], dtype=np.uint8))
    sets = (u64(np.cumsum([0] + [len(x) for x in sel[:8]])), u32(sum(sel[:8], [])))
    return db, walks[:8], reads, arrays, sets, marks, pad


def _rows(db, arrays):
    from oracle import oracle as orc
    sp = orc.bin_reads(arrays["step_off"], arrays["node_id"], [g.range_start for g in db], [g.range_end for g in db])
    so = arrays["step_off"].astype(np.int64)
    rows = []
    for r in range(len(so) - 1):
        s = int(sp[r])
        nodes = (arrays["node_id"][so[r]:so[r + 1]].astype(np.int64) - db[s].range_start).tolist() if s >= 0 else []
        rows.append((s, arrays["flags"][r] == 0, nodes, int(arrays["pstart"][r]), int(arrays["pend"][r])))
    return sp, rows


def _bases_by_rule(db, rows):
    """bases_per_node of the coverage pass for walks that stay inside their species: a single-step read adds pend - pstart; otherwise the first step adds
    len - pstart, an inner step len, the last step what is left of pend - pstart (never below zero), each at the node's first occurrence in the read"""
    out = [np.zeros(g.n_nodes, dtype=np.int64) for g in db]
    for s, counted, nodes, ps, pe in rows:
        if s < 0 or not counted:
            continue
        ln, target = db[s].node_len, pe - ps
        if len(nodes) == 1:
            out[s][nodes[0]] += max(target, 0)
            continue
        assert ps <= ln[nodes[0]]
        seen = 0
        for i, v in enumerate(nodes):
            aln = int(ln[v]) - ps if i == 0 else (max(target, seen) - seen if i == len(nodes) - 1 else int(ln[v]))
            seen += aln
            if v not in nodes[:i]:
                out[s][v] += aln
    return out


def _fixture_holds_the_cases(db, walks, reads, arrays, sets, marks, pad, sp, bases, exp):
    """what the hand-placed walks and reads are meant to be and that no class is empty, from the reference alone"""
    species, table, hap, brk_off, rec = exp
    so, sh = sets
    K = np.diff(so.astype(np.int64))
    assert K.tolist() == [1, 1, 1, 2, 0, 6, 64, 66]
    # the selected walks of species 5 in list order, and where they lie in the tiles
    p5 = sum(len(w) for ws in walks[:5] for w in ws)
    first = {h: p5 + sum(len(w) for w in walks[5][:h]) for h in range(7)}
    e5 = int(so[5])
    assert [len(walks[5][h]) for h in sh[e5:e5 + 6]] == [2 * TILE + 1, TILE, 2, TILE + 1, 18, 1]
    assert first[1] % TILE == 0 and first[2] % TILE == 0 and first[3] % TILE == 1        # h3 begins mid-tile
    e_h3, e_h1, e_h2 = e5, e5 + 1, e5 + 3
    by_entry = {c: rec[int(brk_off[c]):int(brk_off[c + 1])] for c in range(len(sh))}
    steps = lambda c: [r[0] for r in by_entry[c]]
    assert TILE - 1 in steps(e_h2) and (first[2] + TILE - 1) % TILE == TILE - 1          # h2's broken link {1023, 2100} lies on its tile border
    assert TILE - 2 in steps(e_h3) and 2 * TILE - 2 in steps(e_h3) and (first[3] + TILE - 2) % TILE == TILE - 1   # ... and two of h3's on its two
    assert steps(e_h3) == sorted(steps(e_h3)) and sum(1 for c in by_entry if by_entry[c]) >= 3       # at least two strains own break records
    r_border = [r for r in by_entry[e_h2] if r[0] == TILE - 1][0]
    assert r_border[2:4] == (1023, 2100) and r_border[5] == 1 << 3                      # in walk order; private to list position 3
    assert [r for r in by_entry[e_h3] if r[0] == TILE - 2][0][5] == 0b1011              # {1022, 1023}: walked by h3, h1 and h2 (positions 0, 1, 3)
    # u v u: one link at two positions; u u
    assert walks[5][1][:5] == [0, 1, 0, 5, 5] and hap[e_h1, ref.SUPPORT] >= 2 * 2 + 1
    # distinct larger neighbours of a node, over the selected walks of species 5
    nb = {}
    for h in sh[e5:e5 + 6]:
        w = walks[5][h]
        for a, b in zip(w, w[1:]):
            nb.setdefault(min(a, b), set()).add(max(a, b))
    assert len(nb[2150]) == 9 and len(nb[1023]) == 2 and len(nb[1500]) == 1
    # every crossing class and every position class holds something; bit 63 is in use
    assert (species[:, ref.KNOWN:].sum(axis=0) > 0).all() and (species[5, ref.KNOWN:] > 0).all()
    assert (hap[:, ref.CROSSED:ref.SUPPORT].sum(axis=0) > 0).all() and hap[e_h2, ref.PRIVATE_BROKEN] >= 1
    e6 = int(so[6])
    assert any(r[5] == 1 << 63 for r in by_entry[e6 + 63]) and table[6, ref.CORE] == 3 and table[6, ref.CORE_CROSSED] >= 2
    assert table[3, ref.CORE] == table[3, ref.DISTINCT] == 2 and table[5, ref.CORE] == 0
    assert species[4, ref.FOREIGN] == species[4, ref.CROSSINGS] > 0 and not species[7, ref.KNOWN:].any() and species[7, ref.CROSSINGS] > 0
    # an uncrossed link with one end at bases = 0 is open, with both ends covered broken; 2047 is covered by single-step reads only
    assert bases[5][1024] > 0 and bases[5][1025] == 0 and bases[5][2046] > 0 and bases[5][2047] > 0
    assert all(len(r[1]) == 1 for r in reads if r[0] == 5 and 2047 in r[1])
    k = np.diff(arrays["step_off"].astype(np.int64))
    assert {1, 2, 64, 65, 130} <= set(k.tolist())
    for name, at in (("long64", 62), ("long65", 63), ("long130_63", 63), ("long130_64", 64), ("long130_127", 127)):
        nodes = reads[marks[name][0]][1]
        odd = [i for i in range(len(nodes) - 1) if ref.link(nodes[i], nodes[i + 1]) not in (ref.link(10, 11), ref.link(20, 21))]
        assert odd == [at]
    assert (sp < 0).sum() == 2 and ((sp >= 0) & (arrays["flags"] != 0)).sum() >= 3
    assert {reads[i][0] for i in marks["tiny"]} == {0, 1, 2, 3} and sum(len(reads[i][1]) for i in marks["tiny"]) <= 64
    ref.check_identities(species, table, hap, brk_off, [len(walks[s][h]) for s in range(len(db)) for h in sh[int(so[s]):int(so[s + 1])]], so)


def _expected(db, walks, rows, bases, sets):
    return ref.links(walks, [g.node_len for g in db], bases, rows, *sets)


@pytest.fixture(scope="module")
def stage():
    from pantax_amd.engine import Engine
    db, walks, reads, arrays, sets, marks, pad = _build()
    sp, rows = _rows(db, arrays)
    bases = _bases_by_rule(db, rows)
    exp = _expected(db, walks, rows, bases, sets)
    _fixture_holds_the_cases(db, walks, reads, arrays, sets, marks, pad, sp, bases, exp)   # on the CPU, before any GPU run
    eng = Engine(0)
    _resident(eng, db, arrays)
    got_bases = eng.get_node_abundances()[0]
    assert np.array_equal(np.asarray(got_bases).astype(np.int64), np.concatenate(bases))   # the rule above is the coverage pass's
    yield eng, db, walks, arrays, sets, exp
    eng.close()


def _resident(eng, db, arrays, coverage=True):
    a = arrays
    eng.upload_db(db)
    eng.upload_reads(a["step_off"], a["node_id"], a["pstart"], a["pend"], a["qlen"], a["mapq"], a["flags"])
    eng.rcls_profile(want_species=False)
    if coverage:
        eng.trio_nodes_info()
        eng.get_node_abundances(fetch=False)


def _same(got, exp):
    species, table, hap, brk_off, rec = exp
    assert len(got) == 10
    for g, e in zip(got[:4], (species, table, hap, brk_off)):
        assert g.dtype == e.dtype == np.uint64 and g.shape == e.shape
        assert np.array_equal(g, e)
    step, start, node_a, node_b, flank, mask = got[4:]
    assert node_a.dtype == node_b.dtype == np.uint32 and all(x.dtype == np.uint64 for x in (step, start, flank, mask))
    assert list(zip(step.tolist(), start.tolist(), node_a.tolist(), node_b.tolist(), flank.tolist(), mask.tolist())) == rec


def test_stage_call_equals_reference(stage, set_opt):
    eng, db, walks, arrays, sets, exp = stage
    _same(eng.strain_links(*sets), exp)
    set_opt(eng, "read_strain_route", "walk")                                        # every species through the compact walk masks
    _same(eng.strain_links(*sets), exp)


def test_identities_and_cross_identity(stage):
    """the identities of the contract on the device's numbers, and crossings = counted.n_steps - counted.n_reads of the read support pass"""
    eng, db, walks, arrays, sets, exp = stage
    so, sh = sets
    species, table, hap, brk_off = eng.strain_links(*sets)[:4]
    ref.check_identities(species, table, hap, brk_off, [len(walks[s][h]) for s in range(len(db)) for h in sh[int(so[s]):int(so[s + 1])]], so)
    counted = eng.strain_read_support(so, sh, np.ones(len(sh)))[1][:, 0]
    assert np.array_equal(species[:, ref.COUNTED], counted[:, 0]) and np.array_equal(species[:, ref.CROSSINGS], counted[:, 1] - counted[:, 0])
    assert counted[:, 0].sum() > 300
    # known = the sum of support over the distinct links: where one strain walks every link once, that sum is the strain's support
    for s in (0, 1, 2):
        e = int(so[s])
        assert hap[e, ref.LINKS] == table[s, ref.DISTINCT] and hap[e, ref.SUPPORT] == species[s, ref.KNOWN] > 0


def _raw(eng, sets, cap, n_species=None, fill=77):
    """the C call as it is -> (rc, [species, link, hap, brk_off], the six record arrays of max(cap, 1) entries of `fill`)"""
    from pantax_amd import _ffi
    from pantax_amd.engine import p
    so, sh = [np.ascontiguousarray(x) for x in sets]
    S = eng.S
    cs = _ffi.ReadStrainSet(S if n_species is None else n_species, so.ctypes.data, sh.ctypes.data if len(sh) else None, None)
    head = [np.full((S, 6), fill, dtype=np.uint64), np.full((S, 4), fill, dtype=np.uint64), np.full((max(len(sh), 1), 8), fill, dtype=np.uint64),
            np.full(len(sh) + 1, fill, dtype=np.uint64)]
    recs = [np.full(max(cap, 1), fill, dtype=dt) for dt in (np.uint64, np.uint64, np.uint32, np.uint32, np.uint64, np.uint64)]
    rc = eng.lib.pantax_hip_strain_links(eng.ctx, eng.db, eng.reads, C.byref(cs), *[p(x) for x in head], cap, *[p(x) for x in recs])
    return rc, head, recs


def test_cap_protocol_and_arguments(stage):
    eng, db, walks, arrays, sets, exp = stage
    species, table, hap, brk_off, rec = exp
    so, sh = sets
    total = len(rec)
    assert total >= 5
    for cap in (0, total - 1):                                                       # the summaries are written, the record arrays are not touched
        rc, head, recs = _raw(eng, sets, cap)
        assert rc == E_LIMIT
        assert all(np.array_equal(g[:len(e)], e) for g, e in zip(head, (species, table, hap, brk_off)))
        assert all(np.all(x == 77) for x in recs)
    rc, head, recs = _raw(eng, sets, total)                                          # exact
    assert rc == 0 and all(np.array_equal(g[:len(e)], e) for g, e in zip(head, (species, table, hap, brk_off)))
    assert list(zip(*[x.tolist() for x in (recs[0], recs[1], recs[2], recs[3], recs[4], recs[5])])) == rec
    # the argument errors of the read passes, with the outputs left as given
    twice, far = sh.copy(), sh.copy()
    twice[int(so[5]) + 1] = twice[int(so[5])]                                        # a haplotype twice within a species
    far[int(so[0])] = 2                                                              # species 0 has two haplotypes
    for bad, kw in (((so, twice), {}), ((so, far), {}), ((so[:-1], sh), {"n_species": eng.S - 1})):
        rc, head, recs = _raw(eng, bad, total, **kw)
        assert rc == E_INVALID and all(np.all(x == 77) for x in head + recs), bad
    # nothing selected is fine: every crossing is foreign, no links, no records
    z = np.zeros(len(db) + 1, dtype=np.uint64)
    got = eng.strain_links(z, np.zeros(0, dtype=np.uint32))
    assert np.array_equal(got[0][:, :2], species[:, :2]) and np.array_equal(got[0][:, ref.FOREIGN], species[:, ref.CROSSINGS]) and not got[0][:, ref.KNOWN:ref.FOREIGN].any()
    assert not got[1].any() and got[2].shape == (0, 8) and got[3].tolist() == [0] and all(len(x) == 0 for x in got[4:])


def test_state(stage):
    """reads that are not binned and a db without a coverage result of the stage kind are refused; the outputs are left as given"""
    from pantax_amd._ffi import PantaxHipError
    from pantax_amd.engine import Engine
    eng, db, walks, arrays, sets, exp = stage
    a = arrays
    with Engine(0) as e2:
        e2.upload_db(db)
        e2.upload_reads(a["step_off"], a["node_id"], a["pstart"], a["pend"], a["qlen"], a["mapq"], a["flags"])
        rc, head, recs = _raw(e2, sets, 100)                                         # not binned yet
        assert rc == E_STATE and all(np.all(x == 77) for x in head + recs)
        e2.rcls_profile(want_species=False)
        e2.trio_nodes_info()
        rc, head, recs = _raw(e2, sets, 100)                                         # binned, no coverage pass yet
        assert rc == E_STATE and all(np.all(x == 77) for x in head + recs)
        e2.get_node_abundances(fetch=False)
        _same(e2.strain_links(*sets), exp)
        e2.profile_step(np.array([g.genome_len.mean() for g in db], dtype=np.float64))   # a resident step keeps no coverage result of the stage kind
        with pytest.raises(PantaxHipError) as e:
            e2.strain_links(*sets)
        assert e.value.code == E_STATE and "resident step" in str(e.value)
        e2.upload_db(db)                                                             # a new db: the reads were binned against the previous one
        with pytest.raises(PantaxHipError) as e:
            e2.strain_links(*sets)
        assert e.value.code == E_STATE


def test_host_helpers_through_the_binding():
    """link_crossings and link_top of the engine module against the reference (the native check holds their edges)"""
    from pantax_amd.engine import link_crossings, link_top
    masks, known = [1, 1, 2, 0, 3, 3], [1, 0, 0, 0, 0]
    assert link_crossings(masks, known, 2).tolist() == ref.crossings(masks, known, 2) == [1, 1, 1, 2]
    assert link_crossings([1 << 63, 1 << 63], [0], 64).tolist() == [0, 1, 0, 0] and link_crossings([5], [], 3).tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        link_crossings([1, 1], [0], 65)
    flank, start = [5, 9, 5, 9, 1], [40, 30, 10, 20, 0]
    assert link_top(flank, start).tolist() == ref.top(flank, start) == [3, 1, 2, 0, 4]
    assert link_top(flank, start, top=2).tolist() == [3, 1] and link_top([], []).tolist() == []


# ---- the file seam -----------------------------------------------------------------------------------------------------------

HEADER = ["species_taxid", "strain_taxid", "genome_ID", "class", "rank", "n_links", "crossed", "open", "broken", "private", "private_crossed", "private_broken",
          "support", "crossed_fraction", "start", "node_a", "node_b", "flank_depth", "shared_with", "predicted_coverage"]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    yield from seam_world(tmp_path_factory, "pantax_links", 33, 3, 5, 9000, 30000, present_frac=0.6, with_ids=True)


def _frac(n, of):
    return np.float64(n) / np.float64(of) if int(of) else None


def _expected_rows(sset, db, wd, eng, top):
    """the report from the reference and the run's tables: Sel = the rows of strain_abundance.txt in ascending haplotype index; bases_per_node as the
    coverage pass hands it out (pinned against the oracle by the parity tests)"""
    table = _lines(wd / "strain_abundance.txt")[1:]
    names = [g.name for g in sset.species]
    genome_hap = {r[0]: r[0].split("_ASM")[0] for r in _lines(db / "genomes_info.txt")[1:]}
    S = len(names)
    picked = [[] for _ in names]
    for i, t in enumerate(table):
        s = names.index(t[0])
        picked[s].append((sset.species[s].hap_names.index(genome_hap[t[2]]), i))
    picked = [sorted(pk) for pk in picked]
    so, sh = u64(np.cumsum([0] + [len(pk) for pk in picked])), u32([h for pk in picked for h, _ in pk])
    entry_of_row = {i: int(so[s]) + k for s, pk in enumerate(picked) for k, (_, i) in enumerate(pk)}
    a = sset.reads
    arrays = dict(step_off=a.step_off, node_id=a.node_id, pstart=a.pstart, pend=a.pend, flags=np.zeros(a.n_reads, dtype=np.uint8))
    _, read_rows = _rows(sset.species, arrays)
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    flat = np.asarray(eng.get_node_abundances()[0]).astype(np.int64)
    cuts = np.cumsum([0] + [g.n_nodes for g in sset.species])
    bases = [flat[cuts[s]:cuts[s + 1]] for s in range(S)]
    walks = [[g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])].tolist() for h in range(g.n_paths)] for g in sset.species]
    species, link, hap, brk_off, rec = ref.links(walks, [g.node_len for g in sset.species], bases, read_rows, so, sh)
    seq = [r[0] for r in _lines(wd / "ev.tsv")[1:] if r[3] == "total"]       # the species that went through the strain step, in the run's order
    assert len(set(seq)) == len(seq) >= 2 and {t[0] for t in table} <= set(seq)
    rows = []
    for i, t in enumerate(table):
        e, s = entry_of_row[i], names.index(t[0])
        q = hap[e].tolist()
        pc = np.float64(t[3])
        rows.append(t[:3] + ["strain", None] + q + [_frac(q[ref.CROSSED], q[ref.LINKS])] + [None] * 5 + [pc])
        mine = rec[int(brk_off[e]):int(brk_off[e + 1])]
        for k, j in enumerate(ref.top([r[4] for r in mine], [r[1] for r in mine], top)):
            _, start, na, nb, flank, mask = mine[j]
            first = sset.species[s].range_start
            rows.append(t[:3] + ["break", k + 1] + [None] * 9 + [start, first + na, first + nb, flank, bin(mask).count("1"), pc])
    for x in seq:
        s = names.index(x)
        for c, name in enumerate(("links", "core")):
            rows.append([x, None, None, name, None, int(link[s, 2 * c]), int(link[s, 2 * c + 1])] + [None] * 6 + [_frac(link[s, 2 * c + 1], link[s, 2 * c])] + [None] * 6)
        for c, name in enumerate(ref.CROSSING_NAMES):
            rows.append([x, None, None, name] + [None] * 8 + [int(species[s, ref.CROSSINGS + c]), _frac(species[s, ref.CROSSINGS + c], species[s, ref.CROSSINGS])] + [None] * 6)
    return rows, species, hap, rec


def _same_rows(got, exp):
    assert len(got) == len(exp)
    for a, b in zip(got, exp):
        assert len(a) == len(b) == len(HEADER)
        for x, y in zip(a, b):
            if y is None:
                assert x == "-", (a, b)
            elif isinstance(y, np.float64):
                assert np.float64(x) == y, (a, b)
            else:
                assert x == str(y), (a, b)


def test_profile_seam_links(world, capfd, monkeypatch):
    from pantax_amd import _ffi
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng = world
    plain, wd = root / "wd_plain", root / "wd_lk"
    _profile(eng, db, plain, gaf, strain_evidence_file=str(plain / "ev.tsv"))
    _profile(eng, db, wd, gaf, strain_evidence_file=str(wd / "ev.tsv"), strain_links_file=str(wd / "lk.tsv"))
    for f in ("species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt", "ev.tsv"):   # the option changes no table and no other report
        assert open(wd / f, "rb").read() == open(plain / f, "rb").read(), f
    assert not os.path.exists(plain / "lk.tsv")                                     # the report off
    rows = _lines(wd / "lk.tsv")
    assert rows[0] == HEADER
    exp, species, hap, rec = _expected_rows(sset, db, wd, eng, 10)                   # top 0 = the default of 10
    _same_rows(rows[1:], exp)
    assert species[:, ref.KNOWN].sum() > 0 and hap[:, ref.CROSSED].sum() > 0 and len(rec) > 0 and any(r[3] == "break" for r in rows[1:])
    full = open(wd / "lk.tsv", "rb").read()
    # --strain-links-top 1
    w1 = root / "wd_lk_top1"
    _profile(eng, db, w1, gaf, strain_evidence_file=str(w1 / "ev.tsv"), strain_links_file=str(w1 / "lk.tsv"), strain_links_top=1)
    exp1, _, _, _ = _expected_rows(sset, db, w1, eng, 1)
    _same_rows(_lines(w1 / "lk.tsv")[1:], exp1)
    assert all(r[4] == 1 for r in exp1 if r[3] == "break") and len(exp1) < len(exp)
    # beside the read rescue and the segment report: the same file
    wb = root / "wd_lk_beside"
    _profile(eng, db, wb, gaf, strain_links_file=str(wb / "lk.tsv"), strain_rescue_file=str(wb / "rc.tsv"), strain_segments_file=str(wb / "sg.tsv"))
    assert open(wb / "lk.tsv", "rb").read() == full
    # a species-only run writes nothing; the strain-only resume behind it writes the same file
    wr = root / "wd_lk_resume"
    capfd.readouterr()
    _profile(eng, db, wr, gaf, species=True, strain=False, out_binning_file=str(wr / "reads_classification.tsv"), strain_links_file=str(wr / "lk_species_only.tsv"))
    assert not os.path.exists(wr / "lk_species_only.tsv") and "no strain step" in capfd.readouterr().err
    _profile(eng, db, wr, gaf, species=False, strain=True, strain_links_file=str(wr / "lk.tsv"))
    assert open(wr / "lk.tsv", "rb").read() == full
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_lk_cli"
    wc.mkdir()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0",
                        "--strain-links", str(wc / "lk.tsv"), "--strain-links-top", "10"], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc / "lk.tsv", "rb").read() == full
    # several ranks: refused on every rank with the table's wording, before any collective
    for rank in range(2):
        wn = root / ("wd_lk_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, strain_links_file=str(wn / "lk.tsv"))
        assert e.value.code == E_INVALID and "the link support report (strain_links_file) needs one rank and an unsharded ingest (world_size 2)" in str(e.value)
        assert not os.path.exists(wn / "lk.tsv")
    # a caller compiled against the header before these fields: its struct ends behind strain_rescue_top, the report reads as off
    real = _ffi.ProfileExt

    class OldExt(real):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.struct_size = 152

    monkeypatch.setattr(_ffi, "ProfileExt", OldExt)
    wold = root / "wd_lk_old"
    _profile(eng, db, wold, gaf, strain_fit_file=str(wold / "fit.tsv"), strain_links_file=str(wold / "lk.tsv"))
    monkeypatch.setattr(_ffi, "ProfileExt", real)
    assert os.path.exists(wold / "fit.tsv") and not os.path.exists(wold / "lk.tsv")
    assert open(wold / "strain_abundance.txt", "rb").read() == open(wd / "strain_abundance.txt", "rb").read()
