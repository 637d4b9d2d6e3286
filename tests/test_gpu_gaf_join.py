"""GPU tests of two things the device GAF tokenizer (stage_gaf.hip) hands the file seam and nothing else looks at:

  * the joined columns after they GREW between two pieces.  tokenize_piece sizes them from the first piece's density; a denser later piece sends
    joined_reserve to allocate larger columns and copy the present contents across -- with reads in them (J.R > 0), or the step column alone.
  * the verdict "no two reads share an id hash" (ids_distinct), which lets the duplicate-id rule (profile.rs:361-437) return at once: from the hash set
    filled piece by piece, and, when the set was sized too small for the text, from the sort of all hashes + dup_count_kernel.

The texts (tests/helpers.py gaf_join_layout) are cut into pieces of 65536 bytes.  Which route each of them takes was worked out by replaying the piece
cuts and the capacity rule of tokenize_piece on the host; the tests ASSERT the route through the counters of pantax_hip_gaf_ids, so a retuned capacity
rule turns them red instead of blind (then change the layout, not the assertion).  The arrays are compared with oracle/gaf_reader.py and with the id
restatements of tests/helpers.py, never with that replay."""
import bisect

import numpy as np
import pytest

from tests.helpers import gaf_id_hash, gaf_ids_expected, gaf_join_layout, gaf_join_text, gaf_piece_cuts

pytestmark = pytest.mark.gpu

PIECE = 65536
# layout -> (pieces, reads, steps, n_grow_r, n_grow_t, id_check)
ROUTE = {"A": (6, 6020, 12040, 1, 1, 2), "B": (12, 3000, 151500, 0, 2, 1), "C": (5, 6000, 12000, 0, 0, 1), "D": (17, 15300, 15300, 2, 2, 2)}


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def layouts():
    """name -> (lines, text, packed arrays of the gaf_reader oracle, (id_hash, id_off, id_len) restated); computed once, read only"""
    from oracle import gaf_reader
    out = {}
    for name in ROUTE:
        lines = gaf_join_layout(name)
        text = gaf_join_text(lines)
        out[name] = (lines, text, gaf_reader.packed(text), gaf_ids_expected(text))
    return out


def _assert_columns(got, want, ids, text, where):
    """every packed column and id column of `got` equals the expected one; a difference is reported with its first index, the read and the piece it lies in"""
    h, off, ln = ids
    cuts = gaf_piece_cuts(text, PIECE)
    ends = [e for _, e in cuts]
    so = want["step_off"].astype(np.int64)
    R = len(off)

    def place(name, i):
        if R == 0:
            return "no reads"
        r = int(np.searchsorted(so, i, side="right")) - 1 if name == "node_id" else i
        r = min(max(r, 0), R - 1)
        k = bisect.bisect_right(ends, int(off[r]))
        first = int(np.searchsorted(off, cuts[k][0]))
        return "read %d, piece %d of %d (its read %d; bytes %d..%d)" % (r, k, len(cuts), r - first, cuts[k][0], cuts[k][1])
    for name, w in list(want.items()) + [("id_hash", h), ("id_off", off), ("id_len", ln)]:
        g = got[name]
        assert g is not None, (where, name, "missing")
        assert g.dtype == w.dtype, (where, name, g.dtype, w.dtype)
        if g.shape != w.shape:
            raise AssertionError("%s: %s has %d entries, expected %d" % (where, name, len(g), len(w)))
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            i = int(bad[0])
            raise AssertionError("%s: %s differs at %d places, first at index %d (%r, expected %r): %s" % (where, name, len(bad), i, g[i], w[i], place(name, i)))


def _load(eng, tmp_path, text, name="t.gaf"):
    from pantax_amd import io as pio
    p = tmp_path / name
    p.write_bytes(text)
    return pio.load_gaf(p, engine=eng, ids=True)


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_columns_after_growth_host_form(eng, tmp_path, set_opt, layouts, name):
    """pantax_hip_gaf_load_device over a text whose later pieces are denser than the first: all columns are the gaf_reader oracle's, the id columns the
    restated ones (positions in the whole file, not in a piece), and the tokenizer did take the route the layout was built for"""
    set_opt(eng, "gaf_piece_bytes", str(PIECE))
    lines, text, want, ids = layouts[name]
    n_pieces, R, T, grow_r, grow_t, id_check = ROUTE[name]
    assert len(gaf_piece_cuts(text, PIECE)) == n_pieces and len(want["pstart"]) == R and len(want["node_id"]) == T     # the layout is the one described
    got = _load(eng, tmp_path, text)
    route = {k: got[k] for k in ("n_pieces", "n_grow_r", "n_grow_t", "id_check", "ids_distinct")}
    print(name, route)
    assert got["n_pieces"] == n_pieces, route
    assert got["n_grow_r"] == grow_r and got["n_grow_t"] == grow_t, route
    assert got["id_check"] == id_check and got["ids_distinct"] == 1, route
    _assert_columns(got, want, ids, text, "layout " + name)


def test_columns_after_growth_resident_form(eng, tmp_path, set_opt, layouts):
    """pantax_hip_reads_load_gaf with a sparse first piece: the resident reads, whose per-read columns were copied into larger ones on the way, give the
    host columns, the species per read and the coverage integers of the packed upload of the gaf_reader oracle's arrays"""
    import synthdata as synth
    from oracle import gaf_reader
    set_opt(eng, "gaf_piece_bytes", str(PIECE))
    sset = synth.make_set(78, 3, 4, 6000, 60000, with_ids=True)
    p1 = tmp_path / "gen.gaf"
    synth.write_gaf(sset.reads, p1)
    gen = p1.read_bytes().split(b"\n")
    assert gen[-1] == b"" and len(gen) > 1000
    comments = [line for rid, line in layouts["A"][0] if rid is None]
    text = b"\n".join(gen[:20]) + b"\n" + b"".join(comments) + b"\n".join(gen[20:])
    assert len(text) <= 1 << 20
    p = tmp_path / "sparse_head.gaf"
    p.write_bytes(text)
    eng.upload_db(sset.species)
    cols = eng.load_reads_from_gaf(p, ids=True)
    print({k: cols[k] for k in ("n_pieces", "n_grow_r", "n_grow_t", "id_check", "ids_distinct")})
    assert cols["n_grow_r"] >= 1 and cols["n_pieces"] == len(gaf_piece_cuts(text, PIECE))
    assert cols["id_off"] is None and cols["id_len"] is None           # no id spans on this path
    sp, rc, bs, lm, uq = eng.rcls_profile()
    eng.db_reset()
    eng.trio_nodes_info()
    bases, cov, tb, nab = eng.get_node_abundances()
    w = gaf_reader.packed(text)
    h, _, _ = gaf_ids_expected(text)
    for k in ("qlen", "mapq", "flags"):
        assert np.array_equal(cols[k], w[k]), ("oracle", k, int(np.nonzero(cols[k] != w[k])[0][0]) if len(cols[k]) == len(w[k]) else "length")
    assert np.array_equal(cols["id_hash"], h)
    assert cols["ids_distinct"] == (1 if len(set(h.tolist())) == len(h) else 0)
    eng.upload_reads(w["step_off"], w["node_id"], w["pstart"], w["pend"], w["qlen"], w["mapq"], flags=w["flags"])
    sp2, rc2, bs2, lm2, uq2 = eng.rcls_profile()
    eng.db_reset()
    eng.trio_nodes_info()
    bases2, cov2, tb2, nab2 = eng.get_node_abundances()
    assert (sp >= 0).sum() > 1000 and int(np.asarray(cov).sum()) > 0                    # the comparison is about something
    assert np.array_equal(sp, sp2)
    for a, b in ((rc, rc2), (bs, bs2), (lm, lm2), (uq, uq2)):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert np.array_equal(bases, bases2) and np.array_equal(cov, cov2) and np.array_equal(tb, tb2) and nab == nab2


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the verdict
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _read_ids(lines):
    return [rid for rid, _ in lines if rid is not None]


def _piece_of_read(text, off):
    """piece index of every read under the tokenizer's cuts"""
    ends = np.array([e for _, e in gaf_piece_cuts(text, PIECE)], dtype=np.int64)
    return np.searchsorted(ends, off.astype(np.int64), side="right")


def _rename_for(variant, lines, text, ids):
    """{read index: new id} of a variant; every renamed read takes an id of the length it had, except in "first_last", where the LAST read takes the
    first read's id: the text only changes behind the last piece cut"""
    rid = _read_ids(lines)
    R = len(rid)
    h, off, ln = ids
    piece = _piece_of_read(text, off)
    n_pieces = int(piece[-1]) + 1
    same = lambda a, b: len(rid[a]) == len(rid[b])
    if variant == "none":
        return {}
    if variant == "first_last":
        assert piece[0] == 0 and piece[R - 1] == n_pieces - 1 and n_pieces > 1
        return {R - 1: rid[0]}
    if variant == "adjacent":                      # two lines side by side in the middle of a piece
        k = n_pieces // 2
        mine = np.nonzero(piece == k)[0]
        a = int(mine[len(mine) // 2])
        assert same(a, a + 1) and piece[a + 1] == k and a > mine[0] and a + 1 < mine[-1]
        return {a + 1: rid[a]}
    if variant == "cross_piece":                   # the last read of a piece and the first read of the next one
        for k in range(n_pieces // 2, n_pieces - 1):
            a = int(np.nonzero(piece == k)[0][-1])
            if same(a, a + 1):
                assert piece[a + 1] == k + 1
                return {a + 1: rid[a]}
        raise AssertionError("no piece border between two ids of one length")
    if variant == "triple":                        # one id on exactly three reads, pieces apart
        a = R // 3
        others = [b for b in (R // 2, R - 7) if same(a, b)]
        assert len(others) == 2
        return {b: rid[a] for b in others}
    order = np.argsort(h, kind="stable")
    rank = np.empty(R, dtype=np.int64)
    rank[order] = np.arange(R)
    if variant == "rank256":                       # the equal pair at sorted positions 256 m - 1 and 256 m: two blocks' share of dup_count_kernel's grid
        for m in range(1, R // 256):
            a = int(order[256 * m - 1])
            later = [c for c in order[256 * m:].tolist() if same(a, c)]     # a read that sorts behind `a` leaves a's rank alone when it takes a's id
            if not later:
                continue
            ren = {later[0]: rid[a]}
            hs = np.sort(h_after(h, ren, rid))
            if hs[256 * m - 1] == hs[256 * m] and int((hs[1:] == hs[:-1]).sum()) == 1:     # re-derived: the ranks hold behind the rename
                return ren
        raise AssertionError("no pair found for a rank 256 m")
    if variant == "last_ranks":                    # the equal pair at the last two sorted positions
        a = int(order[R - 1])
        c = next(c for c in order[:R - 1].tolist() if same(a, c))
        ren = {c: rid[a]}
        hs = np.sort(h_after(h, ren, rid))
        assert hs[R - 2] == hs[R - 1] and hs[R - 3] != hs[R - 2]
        return ren
    raise KeyError(variant)


def h_after(h, rename, rid):
    out = h.copy()
    for r, new in rename.items():
        out[r] = gaf_id_hash(new)
    return out


VARIANTS = [("C", v) for v in ("none", "first_last", "adjacent", "cross_piece", "triple")] + \
           [("D", v) for v in ("none", "first_last", "adjacent", "cross_piece", "triple", "rank256", "last_ranks")]


@pytest.mark.parametrize("name,variant", VARIANTS)
def test_ids_distinct_verdict(eng, tmp_path, set_opt, layouts, name, variant):
    """ids_distinct is exactly "the id hashes of all rows are pairwise different" -- from the hash set (layout C) and from the sort + dup_count_kernel
    (layout D), for no duplicate and for one duplicate wherever it can hide: in two far pieces, side by side, across a piece border, three times, and
    (sort route) at a block border and at the end of the sorted array"""
    set_opt(eng, "gaf_piece_bytes", str(PIECE))
    from oracle import gaf_reader
    lines, text0, want0, ids0 = layouts[name]
    ren = _rename_for(variant, lines, text0, ids0)
    text = gaf_join_text(lines, ren)
    if variant != "first_last":
        assert len(text) == len(text0) and gaf_piece_cuts(text, PIECE) == gaf_piece_cuts(text0, PIECE)      # ids of one length: the cuts did not move
    else:
        assert gaf_piece_cuts(text, PIECE)[:-1] == gaf_piece_cuts(text0, PIECE)[:-1]
    ids = gaf_ids_expected(text)
    truth = len(set(ids[0].tolist())) == len(ids[0])
    assert truth == (variant == "none")
    got = _load(eng, tmp_path, text)
    route = {k: got[k] for k in ("n_pieces", "n_grow_r", "n_grow_t", "id_check", "ids_distinct")}
    print(name, variant, ren, route)
    assert got["id_check"] == ROUTE[name][5], route
    if name == "D":
        assert got["n_grow_r"] >= 1 and got["n_grow_t"] >= 1, route
    assert got["ids_distinct"] == (1 if truth else 0), (variant, ren, route)
    _assert_columns(got, gaf_reader.packed(text), ids, text, "layout %s, %s" % (name, variant))


@pytest.mark.parametrize("text,distinct,id_check", [
    (b"r1\t150\t0\t150\t+\t>1\t400\t3\t153\t150\t150\t60\n", 1, 0),                                                        # one read: nothing to compare
    (b"r1\t150\t0\t150\t+\t>1\t400\t3\t153\t150\t150\t60\nr1\t150\t0\t150\t+\t>2\t400\t3\t153\t150\t150\t60\n", 0, 1),     # two reads, one id
    (b"r1\t150\t0\t150\t+\t>1\t400\t3\t153\t150\t150\t60\nr2\t150\t0\t150\t+\t>2\t400\t3\t153\t150\t150\t60\n", 1, 1),     # two reads, two ids
], ids=["one_read", "two_reads_one_id", "two_reads_two_ids"])
def test_ids_distinct_of_one_and_two_reads(eng, tmp_path, set_opt, text, distinct, id_check):
    from oracle import gaf_reader
    set_opt(eng, "gaf_piece_bytes", str(PIECE))
    got = _load(eng, tmp_path, text)
    assert got["ids_distinct"] == distinct and got["id_check"] == id_check and got["n_pieces"] == 1
    _assert_columns(got, gaf_reader.packed(text), gaf_ids_expected(text), text, "small")
