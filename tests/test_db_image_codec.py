"""The tests' own reader and writer of the graph image format 4 (tests/hipdb_codec.py), pinned on the host: a hand-written image byte by byte,
and read(write(x)) == x over the corpus of tests/db_image_corpus.py, canonical and valid non-canonical forms.  The GPU tests
(tests/test_gpu_db_image.py) then use it as the reference the library's encoder and the unpacking kernels are compared with."""
import struct

import numpy as np
import pytest

from tests import db_image_corpus as corp
from tests import hipdb_codec as codec


def _same(img, g, L=None):
    assert (img.V, img.H, img.P) == (len(g.node_len), len(g.hap_names), len(g.path_nodes))
    assert img.L == (g.L if L is None else L)
    assert np.array_equal(img.node_len, g.node_len)
    assert np.array_equal(img.path_off, g.path_off)
    assert np.array_equal(img.path_nodes, g.path_nodes)
    assert img.names == g.hap_names


HAND_WALK = [0, 1, 2, 1, 0, 2, 2, 2, 0, 1, 1, 0]          # two haplotypes: 7 + 5 steps
HAND_CODES = [0, 2, 2, 1, 1, 4, 0, 0, 3, 2, 0, 1]         # zigzag of 0 +1 +1 -1 -1 +2 0 0 -2 +1 0 -1


def _hand_image():
    u64 = lambda *v: b"".join(struct.pack("<Q", x) for x in v)
    hdr = b"PTXHIPDB" + bytes([4, 0, 0, 0]) + bytes([1, 0, 0, 0]) + u64(3, 2, 12, 307, 3, 1, 256)
    assert len(hdr) == 72
    x = 0xCBF29CE484222325                                 # FNV-1a, 64 bit, over the header
    for b in hdr:
        x = ((x ^ b) * 0x100000001B3) % (1 << 64)
    img = hdr + bytes(8)                                   # header padded to 80
    img += bytes([5, 0, 0x2C, 0x01, 2, 0]) + bytes(10)     # node_len u16: 5, 300, 2
    img += u64(0, 7, 12) + bytes(8)                        # path_off
    img += bytes(4) + bytes(12)                            # blk_first: 0
    img += bytes([0, 0, 0, 0, 1, 0, 0, 0]) + bytes(8)      # blk_off: 0, 1 (one block, one byte per step)
    img += bytes(HAND_CODES) + bytes(256 - 12)             # payload
    img += b"a\nb" + bytes(13)                             # names
    img += u64(x) + bytes(8)                               # end marker
    assert len(img) == 448
    return img


def test_hand_written_image(tmp_path):
    raw = _hand_image()
    p = tmp_path / "hand.hipdb"
    p.write_bytes(raw)
    img = codec.read_image(str(p))
    assert (img.V, img.H, img.P, img.L, img.flags, img.n_blocks, img.payload_bytes) == (3, 2, 12, 307, 1, 1, 256)
    assert img.node_len.tolist() == [5, 300, 2] and img.path_off.tolist() == [0, 7, 12]
    assert img.blk_first.tolist() == [0] and img.blk_off.tolist() == [0, 1] and img.widths.tolist() == [1]
    assert img.path_nodes.tolist() == HAND_WALK and img.names == ["a", "b"]
    q = tmp_path / "hand2.hipdb"
    codec.write_image(str(q), [5, 300, 2], [0, 7, 12], HAND_WALK, ["a", "b"], 307)
    assert q.read_bytes() == raw
    # the same graph, two bytes per step and u32 lengths: another file, the same content
    codec.write_image(str(q), [5, 300, 2], [0, 7, 12], HAND_WALK, ["a", "b"], 307, widths=2, len16=False)
    wide = codec.read_image(str(q))
    assert wide.same_graph(img) and wide.flags == 0 and wide.widths.tolist() == [2] and wide.payload_bytes == 512
    assert q.read_bytes()[80:92] == struct.pack("<3I", 5, 300, 2)


def test_zigzag_thresholds():
    d = np.array([0, 1, -1, 127, -128, 128, -129, 32767, -32768, 32768, -32769, corp.BIG_V - 1, -(corp.BIG_V - 1)], dtype=np.int64)
    zz = codec.zigzag(d.astype(np.uint32))
    assert zz.tolist() == [0, 2, 1, 254, 255, 256, 257, 65534, 65535, 65536, 65537, 2 * (corp.BIG_V - 1), 2 * (corp.BIG_V - 1) - 1]
    assert np.array_equal(codec.unzigzag(zz), d.astype(np.uint32))
    g = corp.db_thresholds()
    assert codec.minimal_widths(g[0].path_nodes).tolist() == corp.threshold_widths()
    assert codec.minimal_widths(g[1].path_nodes).tolist() == [4] * 5
    wp = corp.db_wide_positions()[0]
    assert codec.minimal_widths(wp.path_nodes).tolist() == [2] * 9 + [4] * 9 + [2] * 9 + [4] * 9


def test_reader_refuses_damage(tmp_path):
    raw = bytearray(_hand_image())
    p = tmp_path / "x.hipdb"

    def refused(data):
        p.write_bytes(bytes(data))
        with pytest.raises(ValueError):
            codec.read_image(str(p))
    refused(raw[:-16])                                     # truncated
    refused(raw + bytes(16))                               # trailing bytes
    for at in (0, 8, 12, 16, 432):                         # magic, version, flags, V (the end marker covers the header), the end marker
        bad = bytearray(raw); bad[at] ^= 0x40
        refused(bad)
    bad = bytearray(raw); bad[148] = 3                     # a block of width 3
    refused(bad)
    g = corp.db_walk_lengths()[8]                          # 13 blocks
    off = np.concatenate([[0], np.cumsum(codec.minimal_widths(g.path_nodes))]).astype(np.uint32)
    assert len(off) == 14
    for k, v in ((13, off[13] + 1), (0, 1), (5, off[4]), (5, off[4] + 8)):     # the last entry, the first, a width of 0, a width of 8
        o = off.copy(); o[k] = v
        codec.write_image(str(p), g.node_len, g.path_off, g.path_nodes, g.hap_names, g.L, blk_off=o)
        with pytest.raises(ValueError):
            codec.read_image(str(p))


@pytest.mark.parametrize("name", sorted(corp.small_corpus()) + ["mixed"])
def test_read_write_roundtrip(name, tmp_path):
    db = corp.corpus()[name] if name == "mixed" else corp.small_corpus()[name]
    rng = np.random.default_rng(5)
    p = str(tmp_path / "g.hipdb")
    n_u32 = 0
    for g in db:
        need = codec.minimal_widths(g.path_nodes)
        canon = None
        for kw in (dict(), dict(widths=2), dict(widths=4), dict(widths=corp.mixed_widths(rng, need)), dict(len16=False)):
            codec.write_image(p, g.node_len, g.path_off, g.path_nodes, g.hap_names, g.L, **kw)
            img = codec.read_image(p)
            _same(img, g)
            if not kw:
                canon = img
                assert np.array_equal(img.widths, need)
                assert img.len16 == (int(g.node_len.max()) < 65536)
                n_u32 += not img.len16
            elif "widths" in kw:
                assert np.array_equal(img.widths, np.maximum(need, kw["widths"]))
            else:
                assert not img.len16
            assert img.same_graph(canon)
    if name in ("lengths", "mixed"):
        assert 0 < n_u32 < len(db)                         # u16 and u32 species in one db


def test_corpus_shapes():
    """the corpus holds what it is meant to hold (the GPU tests rely on it)"""
    wl = corp.db_walk_lengths()
    assert [len(g.path_nodes) for g in wl[:9]] == [1, 255, 256, 257, 511, 512, 513, 1025, 3073]
    assert len(wl[9].hap_names) == 600 and len(wl[9].path_nodes) == 600
    assert wl[10].path_off.tolist() == [0, 256, 512, 1024, 1025]
    ln = corp.db_lengths()
    assert int(ln[0].node_len.max()) == 1 and int(ln[1].node_len.max()) == 65535 and int(ln[2].node_len.max()) == 65536
    assert [len(g.node_len) for g in ln[3:]] == [1, 3, 1023, 1025, 2047, 2049, 4095, 4097, 1024, 5]
    rd = corp.db_random_descending()
    assert set(codec.minimal_widths(rd[0].path_nodes).tolist()) == {4} and set(codec.minimal_widths(rd[1].path_nodes).tolist()) == {2}
    assert np.all(np.diff(rd[2].path_nodes[:3000].astype(np.int64)) < 0)
    mx = corp.db_mixed()
    V = np.array([len(g.node_len) for g in mx])
    big = np.nonzero(V > 100)[0]
    assert len(mx) > 3000 and len(big) == 3 and big[0] > 1000 and big[1] - big[0] > 1000 and len(mx) - big[2] > 800
    for db in corp.corpus().values():
        at = 1
        for g in db:                                       # contiguous ranges that span exactly n_nodes; names in byte order
            assert g.range_start == at and g.range_end - g.range_start + 1 == len(g.node_len)
            at = g.range_end + 1
            assert g.hap_names == sorted(g.hap_names)
