"""tests/hap_pairs_ref.py (the numpy restatement of pantax_hip_db_hap_pairs and of the --db-pairs table, which the GPU tests compare with) pinned on a case
computed by hand: six nodes, four haplotypes, among them an identical pair, a nested pair and distinct pairs."""
from types import SimpleNamespace

import numpy as np

from tests.hap_pairs_ref import HEADER, derived, hap_pairs, species_pairs, table

NODE_LEN = [10, 20, 30, 40, 50, 60]
WALKS = [[0, 1, 2, 3],          # h0
         [3, 2, 1, 0, 1],       # h1: the nodes of h0 in another order, node 1 twice -> identical to h0
         [1, 2],                # h2: a strict subset of h0 -> nested
         [2, 4]]                # h3: shares node 2 with the others, walks node 4 alone -> distinct from all; node 5 is walked by nobody
#       {n_nodes, len} of the nodes both walk
PAIR = [[(4, 100), (4, 100), (2, 50), (1, 30)],
        [(4, 100), (4, 100), (2, 50), (1, 30)],
        [(2, 50), (2, 50), (2, 50), (1, 30)],
        [(1, 30), (1, 30), (1, 30), (2, 80)]]
SPECIES = [(6, 210), (1, 60), (1, 30)]   # total; none: node 5; core: node 2, the only one all four walk


def _graph(name="77"):
    off = np.concatenate([[0], np.cumsum([len(w) for w in WALKS])]).astype(np.uint64)
    return SimpleNamespace(name=name, node_len=np.array(NODE_LEN, dtype=np.int64), path_off=off, path_nodes=np.concatenate(WALKS).astype(np.uint32),
                           hap_names=["h0", "h1", "h2", "h3"], n_paths=4, n_nodes=6)


def test_hand_computed_species():
    pair, sp = species_pairs(NODE_LEN, WALKS)
    assert pair.dtype == sp.dtype == np.uint64 and pair.shape == (4, 4, 2) and sp.shape == (3, 2)
    assert pair.tolist() == [[list(x) for x in row] for row in PAIR]
    assert sp.tolist() == [list(x) for x in SPECIES]
    # the derived quantities and the three classes
    assert derived(pair, 0, 1) == (0, 0, 0, "identical", 1.0)
    assert derived(pair, 0, 2) == (50, 0, 50, "nested", 0.5)
    assert derived(pair, 2, 0) == (0, 50, 50, "nested", 0.5)
    assert derived(pair, 0, 3) == (70, 50, 120, "distinct", np.float64(30) / np.float64(150))
    assert derived(pair, 2, 3) == (20, 50, 70, "distinct", np.float64(30) / np.float64(100))
    # the identities of the header
    for a in range(4):
        for b in range(4):
            assert np.all(pair[a, b] <= np.minimum(pair[a, a], pair[b, b])) and np.all(sp[2] <= pair[a, b]) and np.array_equal(pair[a, b], pair[b, a])
    one, sp1 = species_pairs(NODE_LEN, WALKS[3:])
    assert one.tolist() == [[[2, 80]]] and np.array_equal(one[0, 0], sp1[2]) and sp1.tolist() == [[6, 210], [4, 130], [2, 80]]   # K = 1: pair = core
    none, sp0 = species_pairs(NODE_LEN, [])
    assert none.shape == (0, 0, 2) and sp0.tolist() == [[6, 210], [6, 210], [0, 0]]                                                 # K = 0: all none, no core
    assert species_pairs([0, 0], [[0], [1]])[0].tolist() == [[[1, 0], [0, 0]], [[0, 0], [1, 0]]]
    assert derived(species_pairs([0, 0], [[0], [1]])[0], 0, 1) == (0, 0, 0, "identical", None)                                       # no bases at all: no jaccard


def test_selection_order_and_offsets():
    g = _graph()
    sel_off, sel_hap = np.array([0, 3, 3, 5], dtype=np.uint64), np.array([3, 0, 2, 1, 3], dtype=np.uint32)
    pair_off, pair, sp = hap_pairs([g, g, g], sel_off, sel_hap)
    assert pair_off.tolist() == [0, 9, 9, 13] and pair.shape == (13, 2) and sp.shape == (3, 3, 2)
    want = [[PAIR[a][b] for b in (3, 0, 2)] for a in (3, 0, 2)]
    assert pair[:9].reshape(3, 3, 2).tolist() == [[list(x) for x in row] for row in want]
    assert pair[9:].reshape(2, 2, 2).tolist() == [[[4, 100], [1, 30]], [[1, 30], [2, 80]]]
    assert sp[1].tolist() == [[6, 210], [6, 210], [0, 0]] and sp[0].tolist() == [[6, 210], [1, 60], [1, 30]] and sp[2].tolist() == [[6, 210], [1, 60], [1, 30]]


def test_table_rows():
    g = _graph()
    rows = table([g], lambda g, h: "G" + g.hap_names[h])
    assert rows[0] == HEADER and len(HEADER) == 14 and all(len(r) == 14 for r in rows)
    assert rows[1] == ["77", "Gh0", "Gh1", "identical", "4", "100", "4", "100", "4", "100", "0", "0", "0", 1.0]
    assert rows[2] == ["77", "Gh0", "Gh2", "nested", "4", "100", "2", "50", "2", "50", "50", "0", "50", 0.5]
    assert rows[3][:4] == ["77", "Gh0", "Gh3", "distinct"] and rows[3][8:13] == ["1", "30", "70", "50", "120"]
    assert [tuple(r[1:3]) for r in rows[1:7]] == [("Gh0", "Gh1"), ("Gh0", "Gh2"), ("Gh0", "Gh3"), ("Gh1", "Gh2"), ("Gh1", "Gh3"), ("Gh2", "Gh3")]
    assert rows[7] == ["77", "4", "-", "species", "6", "210", "-", "-", "1", "30", "-", "-", "0", "-"] and len(rows) == 8
    only_identical = table([g], lambda g, h: g.hap_names[h], max_distance=0)
    assert [r[3] for r in only_identical[1:]] == ["identical", "species"] and only_identical[-1][12] == "0"
    near = table([g], lambda g, h: g.hap_names[h], max_distance=50)
    assert [r[3] for r in near[1:]] == ["identical", "nested", "nested", "species"]
    single = SimpleNamespace(name="5", node_len=g.node_len, path_off=np.array([0, 2], dtype=np.uint64), path_nodes=np.array([2, 4], dtype=np.uint32), hap_names=["x"], n_paths=1, n_nodes=6)
    assert table([single], lambda g, h: "x")[1:] == [["5", "1", "-", "species", "6", "210", "-", "-", "2", "80", "-", "-", "-", "-"]]
    wide = SimpleNamespace(name="9", n_paths=257)
    assert table([wide], None)[1:] == [["9", "257", "-", "skipped"] + ["-"] * 10]
