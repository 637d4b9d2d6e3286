"""a9 on the device (hap_rows_pass_kernel x 3, hap_combine_kernel, first_filter_kernel) against the oracle on the crafted cases of
tests/hap_stats_cases.py, read through pantax_hip_strain_hap_stats: the counts of non-zero unique-trio windows exactly, the z-score-filtered mean
unrounded to 1e-12 relative, the first filter's decisions (n_candidates, the `has` bits of unique_trio_nodes_fraction and
frequencies_mean) exactly, the same bits on a second run -- under both routes that file the rows of the unique-trio index (they number them
differently, so chunks and sums see another order).  tests/test_hap_stats_cases.py proves on the CPU that no case sits near a decision boundary
it does not name."""
import numpy as np
import pytest

from tests import hap_stats_cases as hc

pytestmark = pytest.mark.gpu

ROUTES = [None, "path"]       # option trio_rows: rows filed from the visit kernel's records (default) / by the pass over the walks


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _stage_run(eng, case, ref):
    eng.trio_nodes_info(fetch=False)
    eng.get_node_abundances(fetch=False)
    met, info = eng.strain_profiling(ref["absolute"], species_active=ref["keep"], fr=case.fr, shift=case.shift)
    nnz, mf = eng.strain_hap_stats()
    return dict(nnz=nnz.copy(), mf=mf.copy(), has=np.array([met[h].has & 3 for h in range(case.H)], dtype=np.uint32),
                fm=np.array([met[h].frequencies_mean for h in range(case.H)]), ncand=np.array([info[s].n_candidates for s in range(len(case.species))]),
                status=[(info[s].status1, info[s].status2) for s in range(len(case.species))])


def _check(case, ref, got, where):
    st = ref["stat"]
    print("%s: nnz device %s oracle %s" % (where, got["nnz"][st][:12].tolist(), ref["nnz"][st][:12].tolist()))
    want, have = ref["mean_filtered"][st], got["mf"][st]
    rel = np.abs(have - want) / np.maximum(np.abs(want), 1e-300)
    rel[(want == 0.0) & (have == 0.0)] = 0.0
    worst = int(np.argmax(rel)) if len(rel) else 0
    print("%s: mean_filtered max relative difference %.3g (haplotype %d: device %r oracle %r)" % (where, rel.max() if len(rel) else 0.0, np.nonzero(st)[0][worst] if len(rel) else -1,
                                                                                                  have[worst] if len(rel) else 0.0, want[worst] if len(rel) else 0.0))
    assert all(s == (0, 0) for s in got["status"]), got["status"]
    assert np.array_equal(got["nnz"][st], ref["nnz"][st]), np.nonzero(got["nnz"][st] != ref["nnz"][st])[0][:10]
    assert np.all(rel <= 1e-12), [(int(np.nonzero(st)[0][i]), float(have[i]), float(want[i])) for i in np.nonzero(rel > 1e-12)[0][:10]]
    assert np.array_equal(got["ncand"], ref["n_candidates"]), (got["ncand"], ref["n_candidates"])
    assert np.array_equal(got["has"], ref["has"]), np.nonzero(got["has"] != ref["has"])[0][:10]
    kept = st & ((ref["has"] & 2) != 0)
    assert np.array_equal(got["fm"][kept], got["mf"][kept])                     # frequencies_mean is the unrounded filtered mean (profile.rs:1165 / :1180)


@pytest.mark.parametrize("route", ROUTES, ids=["rows", "path"])
@pytest.mark.parametrize("name", [n for n in hc.CASE_NAMES if n not in hc.STEP_CASES])
def test_hap_stats_against_the_oracle(eng, set_opt, name, route):
    case = hc.get_case(name)
    ref = case.reference()
    set_opt(eng, "trio_rows", route)
    eng.upload_db(case.species)
    eng.upload_packed(case.reads)
    sp, rc, bs, lm, uq = eng.rcls_profile()
    assert np.array_equal(sp, ref["sp"]) and np.array_equal(rc, ref["counts"][0])
    big = max(g.n_paths for g in case.species) > 1024
    eng.timing_enable(True)
    eng.timing_reset()
    try:
        got = _stage_run(eng, case, ref)
        t = eng.timing_get()
    finally:
        eng.timing_enable(False)
    # a species of more than 1024 haplotypes accumulates in its chunks' own rows of global partials: the library zero-fills them before each of the three
    # passes under a label of its own, and only then
    assert t["hap_rows_pass_kernel"][0] == 1 and t.get("hap_partials_zero_fill", (0, 0.0))[0] == (3 if big else 0), {k: v for k, v in t.items() if "hap" in k}
    _check(case, ref, got, "%s/%s" % (name, route or "rows"))
    eng.db_reset()
    again = _stage_run(eng, case, ref)
    for k in ("nnz", "mf", "has", "fm", "ncand"):
        assert again[k].tobytes() == got[k].tobytes(), k


@pytest.mark.parametrize("route", ROUTES, ids=["rows", "path"])
def test_a_species_the_species_level_dropped(eng, set_opt, route):
    """The resident step: the species without a genome length is dropped on the device (active = 0), its chunks hand back zero partials without reading
    anything, and its neighbours' statistics are what they are when nothing is dropped."""
    case = hc.get_case("dropped_species")
    ref = case.reference()
    set_opt(eng, "trio_rows", route)
    eng.upload_db(case.species)
    eng.upload_packed(case.reads)
    outs = []
    full_avg = np.array([float(g.genome_len.mean()) for g in case.species])
    for avg in (case.avg_len(), full_avg, case.avg_len()):
        keep, absolute, met, info, passed, s_all, s_pass = eng.profile_step(avg, fr=case.fr, shift=case.shift)
        nnz, mf = eng.strain_hap_stats()
        outs.append(dict(keep=keep.copy(), absolute=absolute.copy(), nnz=nnz.copy(), mf=mf.copy(), has=np.array([met[h].has & 3 for h in range(case.H)], dtype=np.uint32),
                         ncand=np.array([info[s].n_candidates for s in range(len(case.species))])))
    got, full = outs[0], outs[1]
    assert got["keep"].tolist() == [1, 0, 1] and np.array_equal(got["keep"], ref["keep"]) and np.array_equal(got["absolute"], ref["absolute"])
    h0, h1 = int(case.hap_off[1]), int(case.hap_off[2])
    assert not got["nnz"][h0:h1].any() and not got["mf"][h0:h1].any() and not got["has"][h0:h1].any() and got["ncand"][1] == 0
    assert full["keep"].all() and full["nnz"][h0:h1].all() and full["mf"][h0:h1].all()
    st = ref["stat"]
    assert np.array_equal(got["nnz"][st], ref["nnz"][st]) and np.array_equal(got["has"], ref["has"]) and np.array_equal(got["ncand"], ref["n_candidates"])
    assert np.all(np.abs(got["mf"][st] - ref["mean_filtered"][st]) <= 1e-12 * np.abs(ref["mean_filtered"][st]))
    for k in ("nnz", "mf"):                                                    # the neighbours: the same bits with and without the dropped species
        assert got[k][st].tobytes() == full[k][st].tobytes(), k
    for k in ("nnz", "mf", "has", "ncand"):
        assert outs[2][k].tobytes() == got[k].tobytes(), k


def test_hap_stats_need_a_collected_step(eng):
    from pantax_amd._ffi import PantaxHipError
    case = hc.get_case("count_2")
    eng.upload_db(case.species)
    eng.upload_packed(case.reads)
    with pytest.raises(PantaxHipError):
        eng.strain_hap_stats()
