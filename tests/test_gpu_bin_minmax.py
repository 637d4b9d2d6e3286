"""The binning pass of resident reads from the per-slot {min id, max id} filed at upload (bin_mm_kernel, the default) against
the pass that reads the walks (option bin_route=walk: bin_slots_kernel) and against the oracle: species per read in file order and
the four counters per species, integer-exact.  No hook hands the slot records out; the coverage pass gathers them, so the cases
with graphs compare its outputs under both routes (a wrong species, drop code or node base in a slot record changes them)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROUTES = (("minmax", "bin_mm_kernel"), ("walk", "bin_slots_kernel"))
WIDE, N_WIDE, NARROW = 7000, 6, 8      # six species of 7000 ids (room for a walk of 5000 steps), then narrow ones of 8 ids


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _ranges(n_narrow):
    """contiguous ranges from id 1: N_WIDE wide species, then n_narrow narrow ones"""
    width = np.array([WIDE] * N_WIDE + [NARROW] * n_narrow, dtype=np.int64)
    rs = 1 + np.concatenate([[0], np.cumsum(width)[:-1]])
    return rs, rs + width - 1


def _walks(rs, re, seed):
    """the walk shapes of the binning pass, empty walks between them, and a filler of random walks of 1 .. 64 steps (about 20 a walk:
    a wave's 64 slots hold some twenty 64-step rounds of the fill kernel's flat loop, so walks begin in one round and end in the next)"""
    rng = np.random.default_rng(seed)
    u32 = lambda a: np.asarray(a, dtype=np.int64).astype(np.uint32)
    empty = np.zeros(0, np.uint32)
    w = []
    for s in range(N_WIDE):
        b, e = int(rs[s]), int(re[s])
        for k in (1, 2, 63, 64, 65, 128, 4097, 5000):            # 5000 > LONG_HASH / 2: the long fill's plain scan
            w.append(u32(b + 10 + np.arange(k)))                  # the minimum is the first step
            w.append(u32(b + 5500 - np.arange(k)))                # descending (reverse strand): the minimum is the last step
        w += [empty, u32([b + 5, b + 50, b + 7]), u32([b + 9, b + 7, b + 5]), u32([b + 5, b + 9, b + 7]), empty, empty]
        w.append(u32(np.concatenate([b + 100 + np.arange(40), [b + 6000], b + 140 + np.arange(40)])))          # the maximum in the middle
        w.append(u32(np.concatenate([b + 100 + np.arange(2000), [b + 3], b + 2100 + np.arange(2000)])))        # the minimum in the middle of a long walk
        w += [u32([b + 5, b + 6, b + 5, b + 7, b + 6]), u32(np.tile(b + 20 + np.arange(30), 2)), u32(np.tile(b + 20 + np.arange(50), 3))]   # revisits
        w += [u32([b]), u32([e]), u32([b, e]), u32([e, b]), u32(e - np.arange(65)), u32(b + np.arange(64)), u32(b + np.arange(WIDE))]  # on the ends
        w += [u32([b + 5, b + 6, e + 1]), u32([e + 1, b + 5]), u32([b - 1, b]), u32(e - 2 + np.arange(4))]       # one id outside / two species
        w.append(u32(e - 4000 + np.arange(4097)))                 # a long walk that leaves its species by 96 ids
    w += [u32([0]), u32([0, 1, 2]), u32([int(re[-1]) + 1]), u32(int(re[-1]) - 70 + np.arange(80)), empty]         # below the first / above the last range
    top = int(re[-1]) + 40
    for _ in range(7000):
        narrow = rng.random() < 0.15                              # the narrow species get their share of short walks
        k = int(rng.integers(1, 65)) if rng.random() < 0.6 and not narrow else int(rng.integers(1, 8))
        a = int(rng.integers(int(rs[N_WIDE]), top)) if narrow else int(rng.integers(1, top))
        step = rng.integers(0, 3, size=k) * (1 if rng.random() < 0.5 else -1)
        w.append(u32(np.clip(a + np.cumsum(step), 0, top)))
        if rng.random() < 0.05:
            w.append(empty)
    order = rng.permutation(len(w))
    w = [w[i] for i in order]
    if sum(1 for x in w if len(x)) % 64 == 0:                     # the last wave of slots stays partly empty
        w.append(u32([5]))
    assert sum(1 for x in w if len(x)) % 64 != 0 and len(w) <= 20000
    step_off = np.concatenate([[0], np.cumsum([len(x) for x in w])]).astype(np.uint64)
    R = len(w)
    return step_off, np.concatenate(w), rng.integers(50, 20000, size=R), rng.choice([0, 2, 3, 30, 59, 60, 255], size=R)


def _bin_both(eng, set_opt, ref_sp, ref_counts):
    """one binning pass per route; each equals the oracle (hence the other) and ran the kernel it names"""
    out = {}
    eng.timing_enable(True)
    try:
        for route, kernel in ROUTES:
            set_opt(eng, "bin_route", route)
            eng.timing_reset()
            sp, *cnt = eng.rcls_profile()
            ran = eng.timing_get()
            assert kernel in ran and not any(k in ran for _, k in ROUTES if k != kernel), (route, sorted(ran))
            assert np.array_equal(sp, ref_sp), route
            for a, b in zip(cnt, ref_counts):
                assert np.array_equal(a, b), route
            out[route] = (sp, cnt)
    finally:
        eng.timing_enable(False)
    assert np.array_equal(out["minmax"][0], out["walk"][0])
    for a, b in zip(out["minmax"][1], out["walk"][1]):
        assert np.array_equal(a, b)
    return out


@pytest.fixture(scope="module")
def crafted():
    """the crafted reads over 6 + 10 species, and the oracle's answer for them, computed once"""
    from oracle import oracle as orc
    rs, re = _ranges(10)
    step_off, node_id, qlen, mapq = _walks(rs, re, 8)
    ref = orc.bin_reads(step_off, node_id, rs, re)
    return dict(rs=rs, re=re, step_off=step_off, node_id=node_id, qlen=qlen, mapq=mapq, ref=ref, counts=orc.species_counts(ref, qlen, mapq, len(rs)))


def _upload(eng, c, flags=None):
    R = len(c["qlen"])
    eng.upload_reads(c["step_off"], c["node_id"], np.zeros(R), np.ones(R), c["qlen"], c["mapq"], flags)


def test_walk_shapes_sorted_ranges_in_lds(eng, set_opt, crafted):
    c = crafted
    ref = c["ref"]
    k = np.diff(c["step_off"].astype(np.int64))
    assert (ref[k == 0] == -1).all() and (ref[k > 4096] >= 0).any() and (ref[k > 4096] == -1).any() and (ref[k == 1] >= 0).any()
    assert len(set(ref.tolist())) == len(c["rs"]) + 1             # every species and "U"
    eng.upload_ranges(c["rs"], c["re"])
    _upload(eng, c)
    _bin_both(eng, set_opt, ref, c["counts"])


def test_drop_flags_and_their_change(eng, set_opt, crafted):
    """drop flags do not change species or counters (they mark the slot record); set, replaced and binned again"""
    c = crafted
    R = len(c["qlen"])
    eng.upload_ranges(c["rs"], c["re"])
    _upload(eng, c, (np.arange(R) % 5 == 0).astype(np.uint8))
    _bin_both(eng, set_opt, c["ref"], c["counts"])
    eng.set_read_flags((np.arange(R) % 3 == 1).astype(np.uint8) * np.uint8(2))
    _bin_both(eng, set_opt, c["ref"], c["counts"])


def test_same_reads_against_two_dbs(eng, set_opt, crafted):
    """the record filed at upload belongs to the reads, not to a db: a second db with other ranges (the first one's wide species
    cut in two, the rest missing) bins the same resident reads"""
    from oracle import oracle as orc
    c = crafted
    eng.upload_ranges(c["rs"], c["re"])
    _upload(eng, c)
    _bin_both(eng, set_opt, c["ref"], c["counts"])
    rs2 = np.concatenate([c["rs"][:N_WIDE], c["rs"][:N_WIDE] + WIDE // 2])
    re2 = np.concatenate([c["rs"][:N_WIDE] + WIDE // 2 - 1, c["re"][:N_WIDE]])
    ref2 = orc.bin_reads(c["step_off"], c["node_id"], rs2, re2)
    assert not np.array_equal(ref2, c["ref"])
    eng.upload_ranges(rs2, re2)                                   # replaces the db; the reads stay resident
    _bin_both(eng, set_opt, ref2, orc.species_counts(ref2, c["qlen"], c["mapq"], len(rs2)))


def test_more_species_than_the_lds_tables_hold(eng, set_opt):
    """S above BIN_LDS_SPECIES (1024): range tables and counters in global memory"""
    from oracle import oracle as orc
    rs, re = _ranges(1100)
    step_off, node_id, qlen, mapq = _walks(rs, re, 9)
    ref = orc.bin_reads(step_off, node_id, rs, re)
    assert (ref >= N_WIDE).sum() > 100
    eng.upload_ranges(rs, re)
    eng.upload_reads(step_off, node_id, np.zeros(len(qlen)), np.ones(len(qlen)), qlen, mapq)
    _bin_both(eng, set_opt, ref, orc.species_counts(ref, qlen, mapq, len(rs)))


@pytest.mark.parametrize("n_narrow", [10, 1100])
def test_unsorted_overlapping_ranges_take_the_first_match(eng, set_opt, n_narrow):
    """ranges in no order with nested rows (SORTED = false: first match in file order), tables in LDS and in global memory"""
    from oracle import oracle as orc
    rs, re = _ranges(n_narrow)
    step_off, node_id, qlen, mapq = _walks(rs, re, 10)
    perm = np.random.default_rng(1).permutation(len(rs))
    rs2 = np.concatenate([[rs[1] + 100], rs[perm], [rs[0]]])     # a row nested in species 1 in front of it, a row that spans species 0 .. 2 at the end
    re2 = np.concatenate([[rs[1] + 900], re[perm], [re[2]]])
    ref = orc.bin_reads(step_off, node_id, rs2, re2)
    assert (ref == 0).sum() > 0 and (ref == len(rs2) - 1).sum() > 0
    eng.upload_ranges(rs2, re2)
    eng.upload_reads(step_off, node_id, np.zeros(len(qlen)), np.ones(len(qlen)), qlen, mapq)
    _bin_both(eng, set_opt, ref, orc.species_counts(ref, qlen, mapq, len(rs2)))


def _coverage_both(eng, set_opt, ref_sp, ref_counts):
    """binning + coverage pass per route: the outputs that depend on the slot records"""
    got = []
    for route, _ in ROUTES:
        set_opt(eng, "bin_route", route)
        sp, *cnt = eng.rcls_profile()
        assert np.array_equal(sp, ref_sp), route
        for a, b in zip(cnt, ref_counts):
            assert np.array_equal(a, b), route
        eng.db_reset(); eng.trio_nodes_info(fetch=False)
        got.append(eng.get_node_abundances())
    for a, b in zip(got[0][:3], got[1][:3]):
        assert np.array_equal(a, b)
    assert got[0][3] == got[1][3]
    return got[0]


@pytest.mark.parametrize("long_reads", [False, True])
def test_slot_records_feed_the_same_coverage(eng, set_opt, long_reads):
    """a db with graphs: the coverage pass behind either binning route gives the same bases, coverage, trio bases and abort count, with
    drop flags, after their change, and equals the oracle's coverage of the reads the flags keep"""
    import synthdata as synth
    from oracle import oracle as orc
    from tests.helpers import select_reads
    sset = synth.make_set(31 + long_reads, 3, 4, 600 if long_reads else 9000, 60000 if long_reads else 20000, long_reads=long_reads, adversarial_frac=0.01)
    rd = sset.reads
    rs, re = [g.range_start for g in sset.species], [g.range_end for g in sset.species]
    ref = orc.bin_reads(rd.step_off, rd.node_id, rs, re)
    counts = orc.species_counts(ref, rd.qlen, rd.mapq, len(rs))
    if long_reads:
        assert (np.diff(rd.step_off.astype(np.int64)) > 64).any()
    eng.upload_db(sset.species)
    flags = (np.arange(rd.n_reads) % 4 == 0).astype(np.uint8)
    eng.upload_packed(rd, flags)
    a = _coverage_both(eng, set_opt, ref, counts)
    flags2 = (np.arange(rd.n_reads) % 4 == 1).astype(np.uint8)
    eng.set_read_flags(flags2)
    b = _coverage_both(eng, set_opt, ref, counts)
    assert not np.array_equal(a[0], b[0])
    for si, g in enumerate(sset.species):
        G = orc.Graph(g.node_len, g.path_off, g.path_nodes)
        so, nid, ps, pe = select_reads(rd, np.nonzero((ref == si) & (flags2 == 0))[0])
        bases, cov, *_ = orc.node_coverage(G, orc.TrioTable(G), g.range_start, so, nid, ps, pe)
        lo, hi = int(eng.node_off[si]), int(eng.node_off[si + 1])
        assert np.array_equal(b[0][lo:hi], bases) and np.array_equal(b[1][lo:hi], cov)


def test_reads_from_the_device_tokenizer(eng, set_opt, tmp_path):
    """GAF text -> device tokenizer -> resident reads: the grouped copy, and with it the record, is built without host columns"""
    import synthdata as synth
    from oracle import oracle as orc
    sset = synth.make_set(33, 3, 4, 8000, 20000)
    rd = sset.reads
    path = tmp_path / "reads.gaf"
    synth.write_gaf(rd, path)
    ref = orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in sset.species], [g.range_end for g in sset.species])
    eng.upload_db(sset.species)
    cols = eng.load_reads_from_gaf(path)
    assert eng.R == rd.n_reads
    _bin_both(eng, set_opt, ref, orc.species_counts(ref, cols["qlen"], cols["mapq"], len(sset.species)))


def test_reads_from_routed_messages(eng, set_opt, crafted):
    """reads packed for their owner and unpacked there (reads_from_routed) get the record like uploaded ones"""
    from oracle import oracle as orc
    c = crafted
    eng.upload_ranges(c["rs"], c["re"])
    _upload(eng, c)
    eng.rcls_profile()
    rt, nr, nt = eng.route_pack(np.zeros(len(c["rs"]), dtype=np.int32), 1)
    msg = eng.route_messages(rt, 1)[0]
    eng.route_free(rt)
    keep = np.nonzero(c["ref"] >= 0)[0]                           # the binned reads travel, in file order
    assert int(nr[0]) == len(keep)
    eng.reads_from_routed(msg, nr, nt)
    ref = c["ref"][keep]
    _bin_both(eng, set_opt, ref, orc.species_counts(ref, c["qlen"][keep], c["mapq"][keep], len(c["rs"])))
