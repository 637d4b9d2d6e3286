"""The graphs the tests of the device-side graph load are run on (tests/test_db_image_codec.py on the host, tests/test_gpu_db_image.py on the
device): built directly as the objects Engine.upload_db takes, at the shapes where the packed image format 4 and its kernels change behaviour --
block and round borders, the width thresholds of the zigzag deltas, u16 / u32 lengths, many species inside one wave's stretch.  numpy only.

Not covered anywhere: a delta of 2^31 or more (the 32-bit wrap of the zigzag).  It needs two node ids of one species more than 2^31 apart,
hence a species of more than 2^31 nodes: out of reach of a test."""
import numpy as np


class Graph:
    def __init__(self, name, node_len, walks, range_start):
        self.name = name
        self.node_len = np.asarray(node_len, dtype=np.int64)
        walks = [np.asarray(w, dtype=np.uint32) for w in walks]
        self.path_off = np.zeros(len(walks) + 1, dtype=np.uint64)
        self.path_off[1:] = np.cumsum([len(w) for w in walks])
        self.path_nodes = np.concatenate(walks) if walks else np.zeros(0, dtype=np.uint32)
        self.hap_names = ["%s_h%05d" % (name, i) for i in range(len(walks))]          # byte order
        self.range_start = range_start
        self.range_end = range_start + len(self.node_len) - 1
        assert len(self.path_nodes) == 0 or int(self.path_nodes.max()) < len(self.node_len)

    @property
    def L(self):
        return int(self.node_len.sum())


def make_db(specs, prefix):
    """specs: (node_len, walks) per species -> list of Graph with contiguous ranges from 1"""
    out, at = [], 1
    for i, (nl, walks) in enumerate(specs):
        g = Graph("%s%04d" % (prefix, i), nl, walks, at)
        at = g.range_end + 1
        out.append(g)
    return out


def _lens(rng, V, hi=400):
    return rng.integers(1, hi, size=V)


def _backbone(rng, P, V):
    """a walk like a pangenome's: steps of +1 and +2 along the numbering, wrapping at V"""
    return (rng.integers(0, V) + np.cumsum(rng.integers(1, 3, size=P))) % V


def _single_delta_block(start, pos, d, n=256):
    """n steps of +1 from `start`, except the step INTO position pos, which is d"""
    dl = np.ones(n, dtype=np.int64)
    dl[0] = 0
    dl[pos] = d
    w = start + np.cumsum(dl)
    assert w.min() >= 0
    return w


WIDE_POS = (1, 63, 64, 65, 127, 128, 191, 192, 255)          # the borders of the four 64-lane rounds of a block, and their carry
# (delta, bytes per step of a block whose only other deltas are +1)
THRESHOLDS = ((-128, 1), (127, 1), (128, 2), (-129, 2), (-32768, 2), (32767, 2), (32768, 4), (-32769, 4))
BIG_V = (1 << 17) + 3


def db_walk_lengths(seed=11):
    """P = 1, 255, 256, 257, 511, 512, 513, 1024 k + 1 with H = 1; many one-step haplotypes; haplotype borders on block borders and in mid-block"""
    rng = np.random.default_rng(seed)
    specs = []
    for P in (1, 255, 256, 257, 511, 512, 513, 1025, 3073):
        V = 300
        specs.append((_lens(rng, V), [_backbone(rng, P, V)]))
    specs.append((_lens(rng, 700), [[v] for v in rng.integers(0, 700, size=600)]))                       # 600 one-step haplotypes
    specs.append((_lens(rng, 900), [_backbone(rng, n, 900) for n in (256, 256, 512, 1)]))                # borders on block borders
    specs.append((_lens(rng, 900), [_backbone(rng, n, 900) for n in (100, 206, 1, 1, 300, 5, 411)]))     # in mid-block (and one on 1024)
    return make_db(specs, "wl")


def db_thresholds():
    """one block per threshold delta (the other 254 deltas are +1), then ids 0 and V - 1 alternating through three blocks (d = +-(V - 1), V > 2^17:
    the running sum goes below zero and wraps modulo 2^32 between lanes and rounds)"""
    rng = np.random.default_rng(12)
    V = 80000
    walks = [_single_delta_block(40000, 100, d) for d, _ in THRESHOLDS]
    alt = np.where(np.arange(768) % 2 == 0, 0, BIG_V - 1)
    return make_db([(_lens(rng, V), walks), (_lens(rng, BIG_V), [alt, alt[1:513]])], "th")


def threshold_widths():
    return [w for _, w in THRESHOLDS]


def db_wide_positions():
    """the single wide delta of a block at every round border: +1000 (2 bytes) and +70000 (4 bytes), one block per haplotype"""
    rng = np.random.default_rng(13)
    V = 90000
    walks = [_single_delta_block(5000 if d > 0 else 85000, pos, d) for d in (1000, 70000, -1000, -70000) for pos in WIDE_POS]
    return make_db([(_lens(rng, V), walks)], "wp")


def db_random_descending(seed=14):
    rng = np.random.default_rng(seed)
    specs = [
        (_lens(rng, 100000), [rng.integers(0, 100000, size=n) for n in (1500, 1300, 700)]),     # 4-byte blocks
        (_lens(rng, 20000), [rng.integers(0, 20000, size=n) for n in (1111, 2000)]),            # 2-byte blocks
        (_lens(rng, 3000), [np.arange(2999, -1, -1), np.arange(2999, 2000, -3)]),               # strictly descending, 1 byte
        (_lens(rng, 70001), [np.arange(70000, -1, -200), np.arange(70000, 0, -33000)]),         # strictly descending, 2 and 4 bytes
    ]
    return make_db(specs, "rd")


def db_lengths(seed=15):
    """all 1; a maximum of 65535 (u16); one node of 65536 (u32); odd V (the pad entry behind a u16 stretch); V = 1024 k +- 1, 4096 +- 1"""
    rng = np.random.default_rng(seed)
    specs = []
    specs.append((np.ones(777, dtype=np.int64), [_backbone(rng, 300, 777)]))
    nl = _lens(rng, 1001); nl[500] = 65535; nl[1000] = 65535
    specs.append((nl, [_backbone(rng, 257, 1001)]))
    nl = _lens(rng, 1001); nl[0] = 65536
    specs.append((nl, [_backbone(rng, 10, 1001)]))
    for V in (1, 3, 1023, 1025, 2047, 2049, 4095, 4097, 1024, 5):
        specs.append((_lens(rng, V, 65536), [_backbone(rng, 40, V), _backbone(rng, 3, V)]))
    return make_db(specs, "ln")


def db_mixed(seed=16, n_tiny=(1300, 1100, 900)):
    """tiny species (V 1..7, small P) in front of, between and behind large ones; u16 and u32 species in one db: the binary searches of both kernels and
    the per-lane advance of the widening kernel cross many species inside one wave's 1 024 entries and inside four consecutive blocks"""
    rng = np.random.default_rng(seed)

    def tiny(n):
        out = []
        for _ in range(n):
            V = int(rng.integers(1, 8))
            out.append((_lens(rng, V, 3000), [rng.integers(0, V, size=int(rng.integers(1, 6))) for _ in range(int(rng.integers(1, 3)))]))
        return out
    specs = tiny(n_tiny[0])
    specs.append((_lens(rng, 5001), [_backbone(rng, n, 5001) for n in (1700, 1300)]))                       # u16
    specs += tiny(n_tiny[1])
    nl = _lens(rng, 4097); nl[4096] = 70000
    specs.append((nl, [_backbone(rng, 1025, 4097), rng.integers(0, 4097, size=300)]))                       # u32
    alt = np.where(np.arange(600) % 2 == 0, BIG_V - 1, 0)
    specs.append((_lens(rng, BIG_V), [alt, _backbone(rng, 500, BIG_V)]))                                    # u16, 4-byte blocks
    nl = _lens(rng, 8); nl[3] = 1 << 20
    specs.append((nl, [[0, 7, 3]]))                                                                          # a tiny u32 species
    specs += tiny(n_tiny[2])
    return make_db(specs, "mx")


def small_corpus():
    """name -> db; everything but the mixed db (thousands of species)"""
    return {"walk_lengths": db_walk_lengths(), "thresholds": db_thresholds(), "wide_positions": db_wide_positions(),
            "random_descending": db_random_descending(), "lengths": db_lengths()}


def corpus():
    c = small_corpus()
    c["mixed"] = db_mixed()
    return c


def mixed_widths(rng, need):
    """valid widths mixed at random: every block at least as wide as it needs"""
    pick = rng.choice(np.array([1, 2, 4]), size=len(need))
    return np.maximum(need, pick)
