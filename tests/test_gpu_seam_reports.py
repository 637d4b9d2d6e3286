"""GPU test of the six per-strain reports of the file seam together (pantax_amd/csrc/profile_reports.cpp): they share one selection of the group's rows of
strain_abundance.txt and one entry numbering that runs on over the groups.  Each report's own test pins its content against the stage calls with one
or two others beside it; this one pins that all six at once, in one group or in one group a species, write the files each of them writes alone."""
import pytest

from tests.helpers import seam_lines as _lines, seam_profile as _profile, seam_world

pytestmark = pytest.mark.gpu

REPORTS = {"read_strain_file": "rs.tsv", "strain_coverage_file": "ct.tsv", "strain_evidence_file": "ev.tsv", "strain_read_support_file": "sup.tsv",
           "strain_depth_file": "dp.tsv", "strain_near_miss_file": "nm.tsv"}
TABLES = ["species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt"]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    yield from seam_world(tmp_path_factory, "pantax_reports", 32, 4, 5, 30000, 30000, present_frac=0.4, single_strain_every=4, with_ids=True)   # the small world of the seam tests


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_profile_seam_all_reports_at_once(world, set_opt):
    sset, root, db, gaf, eng = world
    # min_cov as test_profile_seam_strain_near_miss chooses it: between the predicted coverages of the table, so that a strain of the sample is dropped at
    # the a15 filter and the near-miss report has a candidate
    _profile(eng, db, root / "wd_all", gaf)
    covs = sorted(float(r[3]) for r in _lines(root / "wd_all" / "strain_abundance.txt")[1:])
    cuts = [int(c) + 1 for c in covs if sum(x < int(c) + 1 for x in covs) >= 1 and sum(x >= int(c) + 1 for x in covs) >= 2]
    assert cuts, covs
    mc = cuts[0]
    # (a) all six in one call
    wa = root / "wd_a"
    _profile(eng, db, wa, gaf, min_cov=mc, **{k: str(wa / v) for k, v in REPORTS.items()})
    table = _lines(wa / "strain_abundance.txt")[1:]
    assert len({r[0] for r in table}) >= 2                                    # later species start at a non-zero entry
    nm = _lines(wa / "nm.tsv")[1:]
    assert any(r[4] == "novel" for r in nm)                                   # at least one candidate row
    # (b) all six in one call, one species a group: the entries of a group start where the groups before ended
    wb = root / "wd_b"
    set_opt(eng, "db_path_steps_max", 1)
    try:
        _profile(eng, db, wb, gaf, min_cov=mc, **{k: str(wb / v) for k, v in REPORTS.items()})
    finally:
        set_opt(eng, "db_path_steps_max", None)
    for f in TABLES + list(REPORTS.values()):
        assert _bytes(wb / f) == _bytes(wa / f), f
    # (c) each report alone
    for k, v in REPORTS.items():
        wc = root / ("wd_c_" + v.split(".")[0])
        _profile(eng, db, wc, gaf, min_cov=mc, **{k: str(wc / v)})
        assert _bytes(wc / v) == _bytes(wa / v), v
        for f in TABLES:
            assert _bytes(wc / f) == _bytes(wa / f), (v, f)
        assert not any((wc / o).exists() for o in REPORTS.values() if o != v)
