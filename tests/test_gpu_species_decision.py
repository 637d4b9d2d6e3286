"""The species decision (species_profiling, profile.rs:299-349) at its edges: `keep` and `absolute` of the resident step (species_profile_kernel: the device
decides) and of Engine.species_profiling (the host decides from the fetched head of rows) against orc.species_profile, on crafted reads over a
three-species db.  keep is compared exactly, absolute bit for bit (one integer-to-f64 quotient).

A read is one node of a species (binned to it) or two nodes of two species ("U"), with chosen read length (GAF column 2) and MAPQ.  The equal-length
verdict covers the first 1000 BINNED rows; in every case reads of other lengths follow the tested position, so that read_count * first_len differs from
the sum of the lengths and a wrong verdict shows in `absolute`.  The kernel preloads a head of 2048 rows and then walks 64 rows at a time: with two
"U" rows before every binned one the 1000th binned read lies at row 2999, in that tail loop.

Reads dropped by flags (upload_packed(flags=...)) are left out: the oracle's reading of the reference has no notion of them.
"""
import numpy as np
import pytest

from tests import hap_stats_cases as hc

pytestmark = pytest.mark.gpu

AVG = np.array([4999.7, 3000.3, 7001.9])


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def species():
    out, start = [], 1
    for s in range(3):
        g = hc.crafted_species(str(s + 1), 2, 3, start)
        out.append(g)
        start = g.range_end + 1
    return out


def B(n, q, s=None, m=60):
    """n binned rows of read length q (species s, or round robin over the three), MAPQ m"""
    return [(i % 3 if s is None else s, q, m) for i in range(n)]


def U(n, q=150):
    return [(-1, q, 60)] * n


def interleave(binned, n_u=2):
    """n_u "U" rows in front of every binned row"""
    out = []
    for r in binned:
        out += U(n_u, 333) + [r]
    return out


TAIL = B(40, 77) + B(25, 212)          # other lengths behind every tested position


def _cases():
    c = {}
    c["equal_1000_then_different"] = B(1000, 150) + B(1, 151) + TAIL                    # the 1001st differs: equal
    c["the_1000th_differs"] = B(999, 150) + B(1, 151) + TAIL                            # rank 999 differs: not equal
    c["u_rows_differ_in_the_head"] = interleave(B(100, 150) + B(1, 151) + B(899, 150) + TAIL)
    c["u_rows_differ_at_rank_999_in_the_tail_loop"] = interleave(B(999, 150) + B(1, 151) + TAIL)
    c["u_rows_differ_at_rank_1000_ignored"] = interleave(B(1000, 150) + B(1, 151) + TAIL)
    for off in (70, 2100):                                                              # the first binned read beyond row 64 / beyond the 2048-row head
        c["first_binned_at_row_%d_equal" % off] = U(off) + B(1000, 200) + TAIL
        c["first_binned_at_row_%d_second_differs" % off] = U(off) + B(1, 200) + B(1, 201) + B(998, 200) + TAIL
    c["fewer_than_1000_binned_equal"] = U(5) + B(500, 150) + U(7)
    c["fewer_than_1000_binned_last_differs"] = U(5) + B(499, 150) + B(1, 90)
    c["no_binned_read"] = U(100)
    c["ten_reads_equal"] = B(10, 150)
    c["ten_reads_one_differs"] = B(9, 150) + B(1, 149)
    c["one_read"] = B(1, 150, s=1)
    c["sixty_three_reads_last_differs"] = U(3) + B(59, 150) + B(1, 151)
    # MAPQ filter (profile.rs:224-245): species 0 has less_multi * 10 == read_count (dropped: `>` is strict), species 1 one more (kept), species 2 reads of
    # MAPQ 3..59 only (uniq_count == 0: dropped)
    c["mapq"] = (B(2, 150, s=0, m=60) + B(18, 150, s=0, m=0) + B(3, 150, s=1, m=60) + B(17, 99, s=1, m=2) + B(5, 150, s=2, m=30) + B(15, 150, s=2, m=61))
    return c


CASES = _cases()
AVGS = {"avg_len_zero_and_negative": np.array([0.0, -5.0, 7001.9])}


def _pack(species, rows, seed=None):
    import synthdata as synth
    starts = [g.range_start for g in species]
    nodes, off = [], [0]
    for i, (s, q, m) in enumerate(rows):
        nodes += [starts[0], starts[1 + i % 2]] if s < 0 else [starts[s] + i % 5]
        off.append(len(nodes))
    n = len(rows)
    ql = np.array([r[1] for r in rows], dtype=np.int64)
    return synth.PackedReads(np.array(off, dtype=np.uint64), np.array(nodes, dtype=np.uint32), np.zeros(len(nodes), dtype=np.uint8), np.zeros(n, dtype=np.int64),
                             np.full(n, 50, dtype=np.int64), ql, np.array([r[2] for r in rows], dtype=np.int64), ql.copy(), [])


def _oracle(species, rd, avg, filtered):
    from oracle import oracle as orc
    sp = orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in species], [g.range_end for g in species])
    counts = orc.species_counts(sp, rd.qlen, rd.mapq, len(species))
    keep, absolute, _ = orc.species_profile(sp, rd.qlen, counts, avg, filtered=filtered)
    return sp, counts, keep, absolute


def _check_both(eng, species, rows, rd, avg, filtered, where):
    sp, counts, keep, absolute = _oracle(species, rd, avg, filtered)
    assert np.array_equal(sp, np.array([r[0] for r in rows], dtype=np.int32)), where          # the rows are binned as they were meant
    got_sp, rc, bs, lm, uq = eng.rcls_profile()
    assert np.array_equal(got_sp, sp) and all(np.array_equal(a, b) for a, b in zip((rc, bs, lm, uq), counts)), where
    hk, ha, _ = eng.species_profiling((rc, bs, lm, uq), avg, filtered=filtered)              # the host's decision
    print("%s: oracle keep %s absolute %s | host %s | counts %s" % (where, keep.tolist(), absolute.tolist(), ha.tolist(), [c.tolist() for c in counts]))
    assert np.array_equal(hk, keep) and ha.tobytes() == absolute.tobytes(), (where, "host", hk, ha, keep, absolute)
    dk, da = eng.profile_step(avg, filtered=filtered)[:2]                                      # the device's decision
    print("%s: device keep %s absolute %s" % (where, dk.tolist(), da.tolist()))
    assert np.array_equal(dk, keep) and da.tobytes() == absolute.tobytes(), (where, "device", dk, da, keep, absolute)
    return keep, absolute, counts


@pytest.mark.parametrize("name", list(CASES))
def test_species_decision_uploaded_reads(eng, species, name):
    rows = CASES[name]
    rd = _pack(species, rows)
    eng.upload_db(species)
    eng.upload_packed(rd)
    keep, absolute, counts = _check_both(eng, species, rows, rd, AVG, True, name)
    binned = [r for r in rows if r[0] >= 0]
    if len(binned) > 1000:                                    # a wrong equal-length verdict would show: the two base counts differ for every species
        assert np.all(counts[0] * binned[0][1] != counts[1])
    if name == "mapq":
        assert keep.tolist() == [0, 1, 0] and counts[2].tolist() == [2, 3, 5] and counts[3].tolist() == [2, 3, 0] and counts[0].tolist() == [20, 20, 20]
        k2, _, _ = _check_both(eng, species, rows, rd, AVG, False, name + "/unfiltered")
        assert k2.tolist() == [1, 1, 1]
    if name == "no_binned_read":
        assert not keep.any()


def test_species_without_a_positive_genome_length_is_dropped(eng, species):
    rows = B(999, 150) + B(1, 151) + TAIL
    rd = _pack(species, rows)
    eng.upload_db(species)
    eng.upload_packed(rd)
    keep, absolute, _ = _check_both(eng, species, rows, rd, AVGS["avg_len_zero_and_negative"], True, "avg_len")
    assert keep.tolist() == [0, 0, 1] and absolute[0] == 0.0 and absolute[1] == 0.0


@pytest.mark.parametrize("name", ["u_rows_differ_in_the_head", "u_rows_differ_at_rank_999_in_the_tail_loop", "u_rows_differ_at_rank_1000_ignored",
                                  "first_binned_at_row_2100_second_differs", "ten_reads_one_differs", "mapq"])
def test_species_decision_device_tokenizer(eng, species, name, tmp_path):
    """the same rows as GAF text through the device tokenizer: the kernel takes the species from the slot records of the grouped reads"""
    import synthdata as synth
    rows = CASES[name]
    rd = _pack(species, rows)
    path = str(tmp_path / "reads.gaf")
    synth.write_gaf(rd, path)
    eng.upload_db(species)
    cols = eng.load_reads_from_gaf(path)
    assert eng.R == len(rows) and np.array_equal(cols["qlen"], rd.qlen) and not cols["flags"].any()
    _check_both(eng, species, rows, rd, AVG, True, name + "/tokenizer")
