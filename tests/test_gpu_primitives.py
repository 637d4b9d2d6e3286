"""The device primitives under every stage (primitives.hpp), each alone against numpy, exactly: the chained exclusive scan (scan_chained.hpp) under each of
its three tiles, forced by the option scan_tile and by the size rule at its edges; the LSD radix sort in its six scatter instantiations (1, 2, 3 key words,
with and without payload), with one and with several tiles per workgroup and with a device-side count below the launch geometry; byte_fill around its 1-MiB
threshold and at every alignment of its head and tail.  The entry points (pantax_hip_scan / _radix_sort / _fill, api_primitives.cpp) take host buffers.

The fused scan functors (GroupCount, TrioFirst, SlowFirst, Pat, Sample) run under the big tiles in tests/test_gpu_trio_plan.py and tests/test_gpu_row_route.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILES = {"small": 2048, "big": 8192, "huge": 16384}
SCAN_BIG_N, SCAN_HUGE_N = 1 << 22, 1 << 26


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------ scan
def scan_ref(x):
    """(exclusive prefix, total) in u32 arithmetic, as the header promises"""
    c = np.cumsum(x, dtype=np.uint32)
    out = np.empty(len(x), dtype=np.uint32)
    out[0] = 0
    out[1:] = c[:-1]
    return out, int(c[-1])


def check_scan(eng, x, tile, in_place=False, what=""):
    out, total, got_tile = eng.scan(x, in_place=in_place)
    ref, ref_total = scan_ref(x)
    assert got_tile == tile, (what, got_tile)
    bad = np.flatnonzero(out != ref)
    assert bad.size == 0, (what, "first difference at item %d of %d: %d, expected %d" % (bad[0], len(x), out[bad[0]], ref[bad[0]]))
    assert total == ref_total, (what, total, ref_total)


def scan_sizes(T):
    # the last two need two and three look-back batches of 64 predecessor tiles
    return [1, 63, 64, 65, T - 1, T, T + 1, 2 * T, 64 * T, 64 * T + 1, 65 * T + 1, 129 * T + 5]


def scan_patterns(rng, n, T, dtype):
    """name -> values: the value patterns of one size"""
    pats = {"random": rng.integers(0, 5, n).astype(dtype), "zero": np.zeros(n, dtype=dtype), "one": np.ones(n, dtype=dtype)}
    edge = np.zeros(n, dtype=dtype)           # one non-zero at the last item of a tile and one at the first item of the next (first and last tile border)
    for k in {1, (n - 1) // T}:
        if k >= 1 and k * T - 1 < n:
            edge[k * T - 1] = 7
        if k >= 1 and k * T < n:
            edge[k * T] = 9
    if n < T:
        edge[n - 1] = 7
    pats["edge"] = edge
    if dtype == np.uint32:                    # sums wrap from the second item on
        pats["wrap"] = rng.integers((1 << 31) - 1000, (1 << 31) + 1000, n).astype(np.uint32)
    return pats


@pytest.mark.parametrize("dtype", [np.uint8, np.uint32], ids=["u8", "u32"])
@pytest.mark.parametrize("tile_name", list(TILES))
def test_scan_under_a_forced_tile(eng, set_opt, tile_name, dtype):
    T = TILES[tile_name]
    set_opt(eng, "scan_tile", tile_name)
    rng = np.random.default_rng(20261101 + T)
    for n in scan_sizes(T):
        for name, x in scan_patterns(rng, n, T, dtype).items():
            check_scan(eng, x, T, what="%s n=%d" % (name, n))
            if dtype == np.uint32 and name in ("random", "wrap"):
                check_scan(eng, x, T, in_place=True, what="%s n=%d in place" % (name, n))


@pytest.fixture(scope="module")
def huge_input():
    """2^26 random bytes and their scan, made once (their sum wraps 32 bits)"""
    x = np.random.default_rng(20261102).integers(0, 256, SCAN_HUGE_N, dtype=np.uint8)
    c = np.cumsum(x, dtype=np.uint32)
    return x, c


def check_scan_prefix_of(eng, huge_input, n, tile):
    x, c = huge_input
    out, total, got_tile = eng.scan(x[:n])
    assert got_tile == tile
    assert out[0] == 0 and np.array_equal(out[1:], c[:n - 1])
    assert total == int(c[n - 1])


@pytest.mark.parametrize("n,tile", [(SCAN_BIG_N - 1, 2048), (SCAN_BIG_N, 8192)], ids=["2^22-1", "2^22"])
def test_scan_auto_rule_at_the_big_edge(eng, huge_input, n, tile):
    """2^22 - 1 items: 2048 tiles of 2048 items, 32 look-back batches"""
    check_scan_prefix_of(eng, huge_input, n, tile)
    x = np.random.default_rng(n).integers(0, 1 << 32, n, dtype=np.uint32)
    check_scan(eng, x, tile, what="u32")
    check_scan(eng, x, tile, in_place=True, what="u32 in place")


@pytest.mark.parametrize("n,no_huge,tile", [(SCAN_HUGE_N - 1, False, 8192), (SCAN_HUGE_N, False, 16384), (SCAN_HUGE_N, True, 8192)],
                         ids=["2^26-1", "2^26", "2^26-no_huge"])
def test_scan_auto_rule_at_the_huge_edge(eng, set_opt, huge_input, n, no_huge, tile):
    if no_huge:
        set_opt(eng, "scan_no_huge", "1")
    check_scan_prefix_of(eng, huge_input, n, tile)


def test_scan_auto_is_the_default_spelled_out(eng, set_opt):
    set_opt(eng, "scan_tile", "auto")
    check_scan(eng, np.arange(5000, dtype=np.uint32), 2048)


def test_scan_workspace_reuse():
    """one ctx, scans of different data whose tile counts go up and down under changing tiles: a state word an earlier scan left must never be taken for a
    published one (the epoch), whatever aggregate it holds"""
    from pantax_amd.engine import Engine
    rng = np.random.default_rng(20261103)
    seq = [("small", 300 * 2048 + 7, "r"), ("huge", 100, "r"), ("big", 40 * 8192 + 3, "r"), ("small", 1, "r"), ("huge", 70 * 16384 + 1, "r"),
           ("small", 50 * 2048, "zero"), ("big", 8192, "r"), ("huge", 3 * 16384, "r"), ("small", 700 * 2048 + 9, "r"), ("big", 5, "r"),
           ("auto", 200 * 2048 + 1, "zero"), ("big", 90 * 8192, "r"), ("auto", 33 * 2048 + 5, "r")]
    with Engine(0) as e:
        for i, (tile_name, n, kind) in enumerate(seq):
            e.set_option("scan_tile", tile_name)
            dtype = np.uint8 if i % 3 == 2 else np.uint32
            x = np.zeros(n, dtype=dtype) if kind == "zero" else rng.integers(0, 200, n).astype(dtype)
            check_scan(e, x, TILES.get(tile_name, 2048), what="scan %d" % i)


def test_scan_unknown_tile_raises(eng, set_opt):
    from pantax_amd._ffi import PantaxHipError
    set_opt(eng, "scan_tile", "tiny")
    with pytest.raises(PantaxHipError, match="scan_tile"):
        eng.scan(np.ones(10, dtype=np.uint32))


# ------------------------------------------------------------------------------------------------ radix sort
SHAPES = [(1, False), (1, True), (2, False), (2, True), (3, False), (3, True)]
SHAPE_IDS = ["%dw%s" % (nw, "+v" if v else "") for nw, v in SHAPES]
LOW16 = [(0, 0), (0, 8)]


def make_records(rng, n, nw, with_v, key0):
    """nw key words, word 0 = key0, the others random; the original index rides in the payload, or, without one, in the last key word beyond the first:
    only the (1, no payload) shape cannot tell equal keys apart"""
    keys = [np.asarray(key0, dtype=np.uint64)] + [rng.integers(0, 1 << 63, n, dtype=np.uint64) for _ in range(nw - 1)]
    idx = np.arange(n)
    if with_v:
        return keys, idx.astype(np.uint32)
    if nw > 1:
        keys[nw - 1] = idx.astype(np.uint64)
    return keys, None


def check_sorted(eng, keys, payload, passes, sort_key, n_actual=None, what=""):
    """the device sort against np.argsort(kind="stable") of sort_key, the value the pass list sorts by; records from n_actual on stay where they were"""
    n = len(keys[0])
    m = n if n_actual is None else n_actual
    got_k, got_v, in_b = eng.radix_sort(keys, passes, payload=payload, n_actual=n_actual)
    assert in_b == (len(passes) % 2 == 1), what
    order = np.concatenate([np.argsort(sort_key[:m], kind="stable"), np.arange(m, n)])
    for w, (g, k) in enumerate(zip(got_k, keys)):
        assert np.array_equal(g, k[order]), (what, "key word %d" % w)
    if payload is not None:
        assert np.array_equal(got_v, payload[order]), (what, "payload")


@pytest.mark.parametrize("nw,with_v", SHAPES, ids=SHAPE_IDS)
def test_sort_is_stable_at_every_small_size(eng, nw, with_v):
    """keys below 2^16, two passes: massive ties from 1025 records on"""
    rng = np.random.default_rng(20261104 + 10 * nw + with_v)
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 4097):
        key0 = rng.integers(0, 1 << 16, n, dtype=np.uint64) if n < 1000 else rng.integers(0, 300, n, dtype=np.uint64) * 211 % (1 << 16)
        keys, v = make_records(rng, n, nw, with_v, key0)
        check_sorted(eng, keys, v, LOW16, key0, what="n=%d" % n)


# 2 097 152: the last size with one 1024-record tile per workgroup; one more: most workgroups' second tile is empty; the third: two ragged tiles each
@pytest.mark.parametrize("n", [2097152, 2097153, 3 * (1 << 20) + 517])
@pytest.mark.parametrize("nw,with_v", [(1, True), (2, False)], ids=["1w+v", "2w"])
def test_sort_is_stable_with_several_tiles_per_workgroup(eng, nw, with_v, n):
    rng = np.random.default_rng(n + nw)
    key0 = rng.integers(0, 1 << 16, n, dtype=np.uint16)
    keys, v = make_records(rng, n, nw, with_v, key0)
    check_sorted(eng, keys, v, LOW16, key0)


@pytest.mark.parametrize("nw,with_v", SHAPES, ids=SHAPE_IDS)
def test_sort_pass_lists(eng, nw, with_v):
    rng = np.random.default_rng(20261105 + 10 * nw + with_v)
    for n in (65, 4097):
        full = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        # a pass at shift 56 (an even number of passes: the result ends in a)
        keys, v = make_records(rng, n, nw, with_v, full)
        check_sorted(eng, keys, v, [(0, 48), (0, 56)], full >> np.uint64(48), what="shift 56, n=%d" % n)
        # a pass list that starts at shift 3 (an odd number: the result ends in b)
        check_sorted(eng, keys, v, [(0, 3), (0, 11), (0, 19)], (full >> np.uint64(3)) & np.uint64(0xFFFFFF), what="shift 3, n=%d" % n)
        # one pass alone
        check_sorted(eng, keys, v, [(0, 24)], (full >> np.uint64(24)) & np.uint64(0xFF), what="one pass, n=%d" % n)
        if nw > 1:
            # a pass list over two words (over three for three-word keys): the second word's low 16 bits below the first word's low 8
            passes = [(1, 0), (1, 8), (0, 0)]
            sort_key = ((full & np.uint64(0xFF)) << np.uint64(16)) | (keys[1] & np.uint64(0xFFFF))
            if nw == 3:
                passes = [(2, 40)] + passes
                sort_key = (sort_key << np.uint64(8)) | ((keys[2] >> np.uint64(40)) & np.uint64(0xFF))
            check_sorted(eng, keys, v, passes, sort_key, what="two words, n=%d" % n)
    # a pass in which all 256 digits occur, then one in which every key has the same digit
    n = 4097
    low = np.concatenate([np.arange(256), rng.integers(0, 256, n - 256)]).astype(np.uint64)
    rng.shuffle(low)
    key0 = low | np.uint64(0x3700)
    assert len(np.unique(key0 & np.uint64(0xFF))) == 256 and len(np.unique(key0 >> np.uint64(8))) == 1
    keys, v = make_records(rng, n, nw, with_v, key0)
    check_sorted(eng, keys, v, LOW16, key0, what="digits")


@pytest.mark.parametrize("n_passes", [2, 3], ids=["ends_in_a", "ends_in_b"])
@pytest.mark.parametrize("nw,with_v", SHAPES, ids=SHAPE_IDS)
def test_sort_device_count_below_the_geometry(eng, nw, with_v, n_passes):
    """the first n_actual records come back sorted, the others as they went in -- on whichever side the result ends"""
    n = 5000
    assert (n // 2) % 1024 != 0
    rng = np.random.default_rng(20261106 + 10 * nw + with_v)
    key0 = rng.integers(0, 1 << 16, n, dtype=np.uint64)
    keys, v = make_records(rng, n, nw, with_v, key0)
    for n_actual in (0, 1, n // 2, n - 1):
        check_sorted(eng, keys, v, [(0, 0), (0, 8), (0, 16)][:n_passes], key0, n_actual=n_actual, what="n_actual=%d" % n_actual)


@pytest.mark.parametrize("frac", ["half", "all_but_one"])
def test_sort_device_count_with_several_tiles_per_workgroup(eng, frac):
    n = 3 * (1 << 20) + 517
    n_actual = n // 2 if frac == "half" else n - 1
    assert (n // 2) % 1024 != 0
    rng = np.random.default_rng(20261107)
    key0 = rng.integers(0, 1 << 16, n, dtype=np.uint16)
    keys, v = make_records(rng, n, 1, True, key0)
    check_sorted(eng, keys, v, LOW16, key0, n_actual=n_actual)


# ------------------------------------------------------------------------------------------------ fill
MIB = 1 << 20
SENTINEL, FRONT = 0x5A, 256      # FRONT sentinel bytes in front of every range (a multiple of 16: `off` alone sets the alignment), 64 behind it


def check_fill(eng, size, off, byte):
    a = FRONT + off
    out = eng.fill(a + size + 64, a, size, byte, SENTINEL)
    what = "size %d off %d byte 0x%02X" % (size, off, byte)
    assert np.count_nonzero(out[:a] != SENTINEL) == 0, what + ": written in front of the range"
    assert np.count_nonzero(out[a + size:] != SENTINEL) == 0, what + ": written behind the range"
    bad = np.flatnonzero(out[a:a + size] != byte)
    assert bad.size == 0, what + ": %d bytes of the range not filled, the first at %d" % (bad.size, bad[0])


# 1 MiB - 1: the runtime's memset; from 1 MiB on the kernel with its head and tail
@pytest.mark.parametrize("size", [MIB - 1, MIB, MIB + 1, MIB + 4111], ids=["1MiB-1", "1MiB", "1MiB+1", "1MiB+4111"])
def test_fill_writes_exactly_its_range(eng, size):
    for off in (0, 1, 15, 16, 17):
        for byte in (0x00, 0xFF, 0xA5):
            check_fill(eng, size, off, byte)


@pytest.mark.parametrize("off", [0, 1, 15, 16, 17])
def test_fill_of_200_mib_writes_exactly_its_range(eng, off):
    """the capped grid: several trips of the four-way unrolled loop and its remainder loop"""
    for byte in (0x00, 0xFF, 0xA5):
        check_fill(eng, 200 * MIB + 5, off, byte)
