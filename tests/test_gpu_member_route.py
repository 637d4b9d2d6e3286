"""Which membership route a strain report takes (member_plan.hpp: member_by_node / member_row, followed by the five launchers), pinned by the library's
timer labels: every case takes one of the five calls under the timers, compares its numbers exactly with the Python reference the call's own test file
uses, and then asserts whether the mask pass of route 2 (label read_strain_mask_kernel) ran.  One set of two species of 8000 bases on either side of the
64-haplotype border, cut into short nodes (mean_len = 8: at the generator's default of 32 such a genome has about 500 nodes, less than a chunk of the
node passes); the references are computed once and shared."""
import numpy as np
import pytest

from tests import depth_ref
from tests.evidence_ref import evidence
from tests.near_miss_ref import near_miss
from tests.test_gpu_read_strains import _bin, _expected as read_strains_expected
from tests.test_gpu_read_support import _reference as read_support_reference

pytestmark = pytest.mark.gpu

MASK = "read_strain_mask_kernel"
CHUNK = 1024        # nodes per chunk of the node evidence and near-miss passes (the depth pass cuts at 2048)
SEED = 20261101

# call -> (its route option, the label of its own pass)
CALLS = {"read_strains": ("read_strain_route", "read_strain_kernel"), "read_support": ("read_strain_route", "read_support_kernel"),
         "evidence": ("evidence_route", "evidence_node_kernel"), "depth": ("depth_route", "depth_hist_kernel"),
         "near_miss": ("near_miss_route", "near_miss_node_kernel")}
# case -> (the selection, the call's route option set to "walk", the mask pass runs)
CASES = {"narrow_default": ("narrow", False, False), "wide_chosen": ("both", False, True), "narrow_walk": ("narrow", True, True)}
# per selection and species: (chosen haplotypes, their weights in the read passes, the near-miss candidates); "narrow" chooses nothing of species 1
PICKS = {"narrow": [([4, 0, 2], [1.0, 2.5, 2.5], [5, 1]), ([], [], [])],
         "both": [([4, 0, 2], [1.0, 2.5, 2.5], [5, 1]), ([64, 0, 33], [7.25, 0.5, 7.25], [63, 1, 30])]}


def _arrays(picks):
    off = lambda k: np.cumsum([0] + [len(p[k]) for p in picks]).astype(np.uint64)
    flat = lambda k, t: np.array(sum((list(p[k]) for p in picks), []), dtype=t)
    return {"sel": (off(0), flat(0, np.uint32)), "w": flat(1, np.float64), "cand": (off(2), flat(2, np.uint32))}


@pytest.fixture(scope="module")
def world():
    """the engine with the set resident behind a coverage pass, the set, and selection -> call -> the reference's numbers; made once, never changed"""
    import synthdata as synth
    from pantax_amd.engine import Engine
    rng = np.random.default_rng(SEED)
    species, start = [], 1
    for s, h in enumerate((6, 65)):
        g = synth.make_species(rng, str(1000 + s), h, 8000, start, "GCF_%06d" % (s + 1), mean_len=8, present_frac=0.3)
        species.append(g)
        start = g.range_end + 1
    reads = synth.make_reads(rng, species, 8000)
    eng = Engine(0)
    eng.upload_db(species)
    eng.upload_packed(reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    bases, cov, _, _ = eng.get_node_abundances()
    R = reads.n_reads
    fill = (np.full(R, 12345, dtype=np.uint32), np.full(R, -7, dtype=np.int32), np.full(R, 0.5))
    sp = _bin(species, reads)
    refs = {}
    for key, picks in PICKS.items():
        a = _arrays(picks)
        cands = (a["sel"][0], a["sel"][1], a["w"])
        refs[key] = {"read_strains": read_strains_expected(species, reads.step_off, reads.node_id, sp, np.ones(R, dtype=bool), *cands, fill),
                     "read_support": read_support_reference(species, reads, np.zeros(R, dtype=np.uint8), cands)[1],
                     "evidence": evidence(species, *a["sel"], cov, bases),
                     "depth": depth_ref.depth(species, *a["sel"], cov, bases),
                     "near_miss": near_miss(species, *a["sel"], *a["cand"], cov, bases)}
    yield eng, species, reads, fill, refs
    eng.close()


def test_the_set_is_what_the_cases_need(world):
    _, species, reads, _, refs = world
    assert [g.n_paths for g in species] == [6, 65]                           # a species on each side of the border of route 1
    assert all(g.n_nodes > CHUNK for g in species)                           # a chunk border inside a species
    assert any(g.n_nodes % CHUNK and g.n_nodes % 64 for g in species)        # a last chunk that ends inside a wave
    assert reads.n_reads == 8000
    for key in PICKS:                                                        # the references have something to say
        r = refs[key]
        assert (r["read_strains"][1] > 0).sum() > 100 and r["read_support"][0][:, 0, 0].sum() > 100
        assert r["evidence"][0][:, 1, 0].sum() > 0 and r["depth"][0][:, 0].sum() > 0 and r["near_miss"][0][:, 0, 0].sum() > 0
    assert refs["both"]["evidence"][0][3:, 0, 0].sum() > 0 and refs["both"]["near_miss"][0][2:, 0, 0].sum() > 0   # entries of the wide species


def _call(eng, which, a, fill):
    if which == "read_strains":
        return eng.read_strains(a["sel"][0], a["sel"][1], a["w"], fill=tuple(np.array(x, copy=True) for x in fill))
    if which == "read_support":
        return eng.strain_read_support(a["sel"][0], a["sel"][1], a["w"])
    if which == "evidence":
        return eng.strain_evidence(*a["sel"])
    if which == "depth":
        return eng.strain_depth(*a["sel"])
    return eng.strain_near_miss(*a["sel"], *a["cand"])


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("which", list(CALLS))
def test_route_and_numbers(world, set_opt, which, case):
    eng, _, _, fill, refs = world
    key, walk, mask_runs = CASES[case]
    option, own = CALLS[which]
    if walk:
        set_opt(eng, option, "walk")
    eng.timing_enable(True)
    eng.timing_reset()
    try:
        got = _call(eng, which, _arrays(PICKS[key]), fill)
        ran = set(eng.timing_get())
    finally:
        eng.timing_enable(False)
    exp = refs[key][which]
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.dtype == e.dtype and g.shape == e.shape
        assert np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g, e.view(np.uint64) if e.dtype == np.float64 else e)
    print("%s, %s: %s" % (which, case, sorted(ran)))
    assert own in ran
    assert (MASK in ran) == mask_runs, sorted(ran)
