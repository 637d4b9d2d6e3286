"""CPU tests of what the host GAF tokenizer reports about read ids (pantax_hip_gaf_ids): the id hash the duplicate-id rule keys on (profile.rs:361-437)
and the place of every id in the file (the binning report writes the ids back from there), against restatements in Python (tests/helpers.py) and the
rows of oracle/gaf_reader.py.  The same restatements check the device tokenizer in tests/test_gpu_gaf_join.py."""
import numpy as np
import pytest

from pantax_amd import io as pio
from tests.helpers import (gaf_id_edge_text, gaf_id_hash, gaf_ids_expected, gaf_join_layout, gaf_join_text, gaf_quirks_text)

# the quirks text of test_device_gaf_tokenizer_equals_host_tokenizer (tests/test_gpu_pipeline.py)
P2_TEXT = (b"@HD\tVN:1.0\n"
           b"r1\t150\t0\t150\t+\t>12<7>300\t400\t3\t153\t150\t150\t60\tNM:i:0\n"
           b"r2\t150\t0\t150\t+\t*\t*\t*\t*\t*\t*\t255\n"
           b"r3\t100\t0\t100\t+\t<5\t30\t20\t10\t100\t100\t*\r\n"
           b"\n"
           b"\r\n"
           b"r5\t99999999999\t0\t1\t+\t>4294967296>7\t1\t99999999999\t5\t1\t1\t300\ta\tb\tc\n"
           b"r6\tx12\t0\t1\t+\t>1>2\t12x\t3\t4\t1\t1\t7\n"
           b"r7\t10\t0\t10\t+\tabc>>9<<10zz11\t5\t\t6\n"
           b"@ comment in the middle\n"
           b"r8\n"
           b"r9\t90\t0\t90\t+\t>8>9\t200\t0\t90")


def _texts():
    out = {"quirks": gaf_quirks_text(), "p2": P2_TEXT, "edges": gaf_id_edge_text()}
    for name in "ABCD":
        out["layout" + name] = gaf_join_text(gaf_join_layout(name))
    return out


def test_id_hash_restatement_known_answers():
    """the restatement itself: FNV-1a-64 of the empty string is the offset basis and of "a" the published af63dc4c8601ec8c; behind them the avalanche"""
    def avalanche(h):
        h ^= h >> 32
        h = (h * 0xd6e8feb86659fd93) & 0xFFFFFFFFFFFFFFFF
        return h ^ (h >> 32)
    assert gaf_id_hash(b"") == avalanche(0xcbf29ce484222325)
    assert gaf_id_hash(b"a") == avalanche(0xaf63dc4c8601ec8c)
    assert gaf_id_hash(b"foobar") == avalanche(0x85944171f73967e8)


def check_ids_against_text(got, text, where):
    """id_hash / id_off / id_len of a tokenizer against the restatements, and the spans against field 0 of the gaf_reader rows (the raw field: the
    reader's null for "*" and the empty field is a property of the value, the span still says where it stands)"""
    from oracle import gaf_reader
    h, off, ln = gaf_ids_expected(text)
    rows = gaf_reader.rows(text)
    assert len(rows) == len(h), where
    for name, want in (("id_hash", h), ("id_off", off), ("id_len", ln)):
        g = got[name]
        assert g is not None and g.dtype == want.dtype and g.shape == want.shape, (where, name)
        if not np.array_equal(g, want):
            i = int(np.nonzero(g != want)[0][0])
            raise AssertionError("%s: %s differs first at read %d: %r, expected %r (id %r)" % (where, name, i, g[i], want[i], text[int(off[i]):int(off[i] + ln[i])]))
    for i, r in enumerate(rows):
        raw = text[int(got["id_off"][i]):int(got["id_off"][i]) + int(got["id_len"][i])]
        assert raw == (r[0] if r[0] is not None else raw) and (r[0] is not None or raw in (b"", b"*")), (where, i, raw, r[0])


@pytest.mark.parametrize("name", ["quirks", "p2", "edges", "layoutA", "layoutB", "layoutC", "layoutD"])
def test_host_tokenizer_ids(tmp_path, name):
    text = _texts()[name]
    p = tmp_path / (name + ".gaf")
    p.write_bytes(text)
    for nt in (1, 3):
        got = pio.load_gaf(p, n_threads=nt, ids=True)
        check_ids_against_text(got, text, (name, nt))
        # the host tokenizer decides nothing about duplicates and takes no route
        assert got["ids_distinct"] == -1 and got["id_check"] == 0
        assert got["n_pieces"] == 0 and got["n_grow_r"] == 0 and got["n_grow_t"] == 0


def test_edge_ids_are_the_edges():
    """the edge text does hold ids of 0, 1, 7, 8 and 9 bytes and lines without a tab"""
    text = gaf_id_edge_text()
    _, off, ln = gaf_ids_expected(text)
    assert {0, 1, 7, 8, 9} <= set(ln.tolist())
    ids = [text[int(o):int(o + n)] for o, n in zip(off, ln)]
    assert b"notab" in ids and b"crlf_no_tab" in ids and ids[-1] == b"lastline_without_tab" and ids[0] == b""


def test_ids_view_of_an_empty_file(tmp_path):
    p = tmp_path / "empty.gaf"
    p.write_bytes(b"")
    got = pio.load_gaf(p, ids=True)
    assert len(got["id_hash"]) == 0 and len(got["id_off"]) == 0 and len(got["id_len"]) == 0 and got["ids_distinct"] == -1
