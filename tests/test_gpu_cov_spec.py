"""The short-read coverage kernel's speculative node record (stage_cov.hip, PF3): the record of a step's node is requested a round ahead at the
delta of the ITEM's species guess -- species and delta of the first slot of the item's first live group, found by the window probe -- and level 3
checks every lane's species against the guess; a wave that holds a read of another species takes the old loads.  Option cov_spec=miss replaces the guess
by a species no read has, so every wave takes the fallback: both ways must give the oracle's results BIT FOR BIT.

The corpus, the stage calls and the comparison are those of tests/test_gpu_cov_walk_edges.py (imported); what this file adds:
  shapes      on / miss under the default shape, covf_shape 182, 2423, 2823, 443 (U = 1, 2, 4) and cov_item_groups 1 and 7 (items shorter than the
              workgroup has waves: the prologue's requests target repeat groups)
  gapped      the same corpus with species B 2048 * 3 + 37 and species C 2048 * 7 + 5 ids higher: three DIFFERENT deltas, border blocks that no longer
              touch -- in the plain corpus the id ranges are contiguous, so every species has the same delta and a wrong one would be invisible
  deselected  each species deselected in turn: the guess comes from the first ACTIVE species of an item (the `border` class: items that hold reads of two
              species), the lanes of the deselected one beside it take the fallback and contribute nothing
  no trio     with_trio=False
"""
import dataclasses

import numpy as np
import pytest

from tests import cov_walk_cases as cw
from tests import test_gpu_cov_walk_edges as we
from tests.helpers import oracle_coverage
from tests.test_gpu_cov_walk_edges import eng, world  # noqa: F401  (module fixtures: the engine; the corpus with the oracle's binning and coverage)

pytestmark = pytest.mark.gpu

SPEC = ("on", "miss")
SHAPES = [("default", {})]
SHAPES += [("covf_shape_%d" % c, {"covf_shape": c}) for c in (182, 2423, 2823, 443)]
SHAPES += [("cov_item_groups_%d" % n, {"cov_item_groups": n}) for n in (1, 7)]
GAP_B, GAP_C = cw.BLOCK * 3 + 37, cw.BLOCK * 7 + 5


def _run(eng, set_opt, spec, species, rd, ref_sp, ref, options=(), species_active=None, with_trio=True, flags=None):
    for opt, value in dict(options).items():
        set_opt(eng, opt, value)
    set_opt(eng, "cov_spec", spec)
    eng.upload_db(species)
    eng.upload_packed(rd, flags=flags)
    sp, bases, cov, tb, nab, ran = we._timed_coverage(eng, species_active=species_active, with_trio=with_trio)
    assert np.array_equal(sp, ref_sp)
    we._check(eng, ref, bases, cov, tb, nab, with_trio=with_trio)
    assert ran & we.LABELS == we.DEFAULT, sorted(ran & we.LABELS)
    return bases, cov, tb


@pytest.mark.parametrize("spec", SPEC)
@pytest.mark.parametrize("name,options", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes(eng, world, set_opt, name, options, spec):
    species, rd, classes, ref_sp, ref = world
    _run(eng, set_opt, spec, species, rd, ref_sp, ref, options)


def gapped(species, rd):
    """B's ids -- its range and every read id inside it -- GAP_B higher, C's GAP_C higher: nothing local to a species changes"""
    A, B, C = species
    ids = rd.node_id.astype(np.int64)
    in_b = (ids >= B.range_start) & (ids <= B.range_end)
    in_c = (ids >= C.range_start) & (ids <= C.range_end)
    assert (in_b | in_c | ((ids >= A.range_start) & (ids <= A.range_end))).all()
    sp = [A, dataclasses.replace(B, range_start=B.range_start + GAP_B, range_end=B.range_end + GAP_B),
          dataclasses.replace(C, range_start=C.range_start + GAP_C, range_end=C.range_end + GAP_C)]
    return sp, dataclasses.replace(rd, node_id=(ids + GAP_B * in_b + GAP_C * in_c).astype(np.uint32))


@pytest.fixture(scope="module")
def gap_world(world):
    from oracle import oracle as orc
    species, rd, classes, ref_sp, ref = world
    sp_g, rd_g = gapped(species, rd)
    starts, ends = [g.range_start for g in sp_g], [g.range_end for g in sp_g]
    # three different deltas (node index - id), and gaps of whole blocks between the ranges: the border blocks no longer touch
    node_off = np.concatenate([[0], np.cumsum([g.n_nodes for g in sp_g])])
    assert len({int(node_off[i]) - starts[i] for i in range(3)}) == 3
    assert all(starts[i + 1] // cw.BLOCK > ends[i] // cw.BLOCK + 1 for i in range(2))
    gsp = orc.bin_reads(rd_g.step_off, rd_g.node_id, starts, ends)
    assert np.array_equal(gsp, ref_sp)                                   # every read keeps its species ...
    assert len(classes["control_u"]) == 2 and (gsp[classes["control_u"]] == -1).all()    # ... and the walks that leave theirs still do
    gref = oracle_coverage(sp_g, rd_g, gsp)                              # the oracle, rerun on the gapped corpus
    for (T, b, c, t, na), (T0, b0, c0, t0, na0) in zip(gref, ref):       # (nothing local to a species moved)
        assert np.array_equal(b, b0) and np.array_equal(c, c0) and np.array_equal(t, t0) and na == na0
    return sp_g, rd_g, gsp, gref


@pytest.mark.parametrize("spec", SPEC)
def test_gapped_ranges(eng, gap_world, set_opt, spec):
    sp_g, rd_g, gsp, gref = gap_world
    _run(eng, set_opt, spec, sp_g, rd_g, gsp, gref)


@pytest.fixture(scope="module")
def deselected_refs(world):
    species, rd, classes, ref_sp, ref = world
    out = {}
    for off in range(3):
        active = np.ones(3, dtype=np.uint8)
        active[off] = 0
        out[off] = (active, oracle_coverage(species, rd, np.where(active[np.maximum(ref_sp, 0)] == 1, ref_sp, -1)))
    return out


@pytest.mark.parametrize("spec", SPEC)
@pytest.mark.parametrize("off", (0, 1, 2), ids=("A_off", "B_off", "C_off"))
def test_border_with_a_species_deselected(eng, world, deselected_refs, set_opt, off, spec):
    """A off: the A|B border item's first species is deselected -- the guess is B's; B off: the other species of that item, and the first of the B|C
    item; C off: the other species of the B|C item.  Nothing of the deselected species is touched, its neighbours in the same waves are complete."""
    species, rd, classes, ref_sp, ref_all = world
    active, ref = deselected_refs[off]
    border_sp = set(ref_sp[classes["border"]].tolist())
    assert border_sp == {0, 1, 2}                                         # reads of every species among the border class
    assert not ref[off][1].any() and not ref[off][2].any() and not ref[off][3].any() and ref[off][4] == 0
    assert all(int(ref[s][1].sum()) > 0 and int(ref[s][3].sum()) > 0 for s in range(3) if s != off)
    bases, cov, tb = _run(eng, set_opt, spec, species, rd, ref_sp, ref, species_active=active)
    lo, hi = int(eng.node_off[off]), int(eng.node_off[off + 1])
    assert not bases[lo:hi].any() and not cov[lo:hi].any()


def test_without_trio(eng, world, set_opt):
    species, rd, classes, ref_sp, ref = world
    bases, cov, tb = _run(eng, set_opt, "on", species, rd, ref_sp, ref, with_trio=False)
    assert tb is None
