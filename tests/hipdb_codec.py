"""An independent reader and writer of the device-ready graph image, `.hipdb` format 4, for the tests (numpy only).

Written from the layout comment at the top of pantax_amd/csrc/db_image.cpp and the description of the packed walks in
common.hpp ("Round 6 (image format 4)"), statement by statement.  It shares no code with the library and never calls it, so a
test that compares the two compares two implementations of one format.

Layout (little endian; the header and every section padded to 16 bytes):
    header  : "PTXHIPDB", u32 version (4), u32 flags (bit 0: node lengths as u16), u64 V, H, P, L, name_bytes, n_blocks, payload_bytes
    node_len  u16/u32 [V]
    path_off  u64 [H + 1]          walk offsets local to the species, path_off[0] = 0, path_off[H] = P
    blk_first u32 [n_blocks]       first node id of every block of 256 consecutive positions of the concatenated walks
    blk_off   u32 [n_blocks + 1]   payload offset of every block in units of 256 bytes; a block's width in bytes per step is the difference
    payload                        per block 256 zigzag deltas of 1, 2 or 4 bytes (the first is 0, the tail behind P is 0)
    names                          '\\n'-joined haplotype names
    u64 end marker                 FNV-1a (64 bit) over the 72 header bytes
A delta is the 32-bit difference of two consecutive node ids (modulo 2^32), zigzag coded: (d << 1) ^ (d >> 31, arithmetic).
"""
import struct

import numpy as np

MAGIC = b"PTXHIPDB"
VERSION = 4
FLAG_LEN16 = 1
BLOCK = 256          # positions per block
UNIT = 256           # bytes per unit of blk_off
HEADER = struct.Struct("<8sII7Q")      # 72 bytes
assert HEADER.size == 72


def _pad16(n):
    return (n + 15) & ~15


def fnv1a64(data):
    x = 0xCBF29CE484222325
    for b in data:
        x = ((x ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return x


def _sections(len16, V, H, n_blocks, payload_bytes, name_bytes):
    """byte offset of every section, and the file size"""
    at = _pad16(HEADER.size)
    out = {}
    for name, nbytes in (("node_len", (2 if len16 else 4) * V), ("path_off", 8 * (H + 1)), ("blk_first", 4 * n_blocks), ("blk_off", 4 * (n_blocks + 1)),
                         ("payload", payload_bytes), ("names", name_bytes), ("end", 8)):
        out[name] = at
        at += _pad16(nbytes)
    out["total"] = at
    return out


def zigzag(d):
    """uint32 differences (two's complement) -> zigzag codes, uint32"""
    d = np.asarray(d, dtype=np.uint32)
    sign = (d.astype(np.int32) >> 31).astype(np.uint32)           # 0 or 0xFFFFFFFF
    return ((d << np.uint32(1)) & np.uint32(0xFFFFFFFF)) ^ sign


def unzigzag(zz):
    zz = np.asarray(zz, dtype=np.uint32)
    return (zz >> np.uint32(1)) ^ (np.uint32(0) - (zz & np.uint32(1)))


def block_codes(path_nodes):
    """-> (blk_first [n_blocks] uint32, codes [n_blocks, 256] uint32): the zigzag deltas of every block, zero in slot 0 and behind P"""
    w = np.asarray(path_nodes, dtype=np.uint32)
    P = len(w)
    nb = (P + BLOCK - 1) // BLOCK
    padded = np.zeros(nb * BLOCK, dtype=np.uint32)
    padded[:P] = w
    diff = np.zeros(nb * BLOCK, dtype=np.uint32)
    diff[1:P] = w[1:] - w[:-1]                                   # modulo 2^32
    codes = zigzag(diff).reshape(nb, BLOCK).copy()
    codes[:, 0] = 0
    return padded.reshape(nb, BLOCK)[:, 0].copy(), codes


def minimal_widths(path_nodes):
    _, codes = block_codes(path_nodes)
    mx = codes.max(axis=1) if len(codes) else np.zeros(0, dtype=np.uint32)
    return np.where(mx < 256, 1, np.where(mx < 65536, 2, 4)).astype(np.int64)


class Image:
    """what read_image returns; == compares everything a graph is (lengths, offsets, walks, names, V, H, P, L)"""
    FIELDS = ("V", "H", "P", "L", "node_len", "path_off", "path_nodes", "names")

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def same_graph(self, other):
        for f in self.FIELDS:
            a, b = getattr(self, f), getattr(other, f)
            if isinstance(a, np.ndarray):
                if a.shape != b.shape or not np.array_equal(a, b):
                    return False
            elif a != b:
                return False
        return True


def read_image(path):
    raw = open(path, "rb").read()
    if len(raw) < HEADER.size:
        raise ValueError("too short for a header")
    hdr = raw[:HEADER.size]
    magic, version, flags, V, H, P, L, name_bytes, n_blocks, payload_bytes = HEADER.unpack(hdr)
    if magic != MAGIC:
        raise ValueError("magic")
    if version != VERSION:
        raise ValueError("version %d" % version)
    if flags & ~FLAG_LEN16:
        raise ValueError("unknown flags %#x" % flags)
    len16 = bool(flags & FLAG_LEN16)
    if n_blocks != (P + BLOCK - 1) // BLOCK:
        raise ValueError("n_blocks %d for %d steps" % (n_blocks, P))
    if payload_bytes % UNIT or not (BLOCK * n_blocks <= payload_bytes <= 4 * BLOCK * n_blocks):
        raise ValueError("payload_bytes %d for %d blocks" % (payload_bytes, n_blocks))
    sec = _sections(len16, V, H, n_blocks, payload_bytes, name_bytes)
    if sec["total"] != len(raw):
        raise ValueError("sections need %d bytes, the file has %d" % (sec["total"], len(raw)))
    if struct.unpack_from("<Q", raw, sec["end"])[0] != fnv1a64(hdr):
        raise ValueError("end marker")
    node_len = np.frombuffer(raw, dtype="<u2" if len16 else "<u4", count=V, offset=sec["node_len"]).astype(np.int64)
    path_off = np.frombuffer(raw, dtype="<u8", count=H + 1, offset=sec["path_off"]).astype(np.uint64)
    if int(path_off[0]) != 0 or int(path_off[-1]) != P or np.any(path_off[1:] < path_off[:-1]):
        raise ValueError("path_off")
    blk_first = np.frombuffer(raw, dtype="<u4", count=n_blocks, offset=sec["blk_first"]).astype(np.uint32)
    blk_off = np.frombuffer(raw, dtype="<u4", count=n_blocks + 1, offset=sec["blk_off"]).astype(np.uint32)
    widths = np.diff(blk_off.astype(np.int64))
    if int(blk_off[0]) != 0 or int(blk_off[-1]) * UNIT != payload_bytes or not np.all(np.isin(widths, (1, 2, 4))):
        raise ValueError("blk_off")
    walk = np.zeros(n_blocks * BLOCK, dtype=np.uint32)
    for b in range(n_blocks):
        w = int(widths[b])
        zz = np.frombuffer(raw, dtype={1: "<u1", 2: "<u2", 4: "<u4"}[w], count=BLOCK, offset=sec["payload"] + int(blk_off[b]) * UNIT).astype(np.uint32)
        d = unzigzag(zz)
        walk[b * BLOCK:(b + 1) * BLOCK] = blk_first[b] + np.cumsum(d, dtype=np.uint32)     # modulo 2^32
    names_raw = raw[sec["names"]:sec["names"] + name_bytes]
    names = [] if H == 0 else [x.decode() for x in names_raw.split(b"\n")]
    if len(names) != H:
        raise ValueError("%d names for %d haplotypes" % (len(names), H))
    return Image(V=V, H=H, P=P, L=L, flags=flags, len16=len16, node_len=node_len, path_off=path_off, blk_first=blk_first, blk_off=blk_off,
                 widths=widths, path_nodes=walk[:P].copy(), names=names, n_blocks=n_blocks, payload_bytes=payload_bytes)


def write_image(path, node_len, path_off, path_nodes, names, L, widths=None, len16=None, blk_off=None):
    """Canonical by default: the minimal width of every block, u16 lengths iff every length is below 2^16.
    widths: an int (every block at least that wide) or one width per block (none below what the block needs) -- valid, not canonical.
    len16=False: u32 lengths where u16 would do (True where a length does not fit is an error).
    blk_off: DAMAGE -- this table is written in place of the true one (same number of entries); everything else stays valid."""
    node_len = np.asarray(node_len, dtype=np.int64)
    path_off = np.asarray(path_off, dtype=np.uint64)
    path_nodes = np.asarray(path_nodes, dtype=np.uint32)
    V, H, P = len(node_len), len(path_off) - 1, len(path_nodes)
    assert int(path_off[0]) == 0 and int(path_off[-1]) == P and len(names) == H
    fits16 = V == 0 or int(node_len.max()) < 65536
    if len16 is None:
        len16 = fits16
    if len16 and not fits16:
        raise ValueError("a length does not fit 16 bits")
    blk_first, codes = block_codes(path_nodes)
    nb = len(blk_first)
    need = minimal_widths(path_nodes)
    if widths is None:
        w = need
    elif np.isscalar(widths):
        w = np.maximum(need, int(widths))
    else:
        w = np.asarray(widths, dtype=np.int64)
        if len(w) != nb or np.any(w < need) or not np.all(np.isin(w, (1, 2, 4))):
            raise ValueError("widths")
    true_off = np.zeros(nb + 1, dtype=np.uint32)
    true_off[1:] = np.cumsum(w * (BLOCK // UNIT))
    payload = b"".join(codes[b].astype({1: "<u1", 2: "<u2", 4: "<u4"}[int(w[b])]).tobytes() for b in range(nb))
    assert len(payload) == int(true_off[-1]) * UNIT
    if blk_off is not None:
        blk_off = np.asarray(blk_off, dtype=np.uint32)
        assert len(blk_off) == nb + 1
    joined = "\n".join(names).encode()
    assert all("\n" not in n for n in names)
    hdr = HEADER.pack(MAGIC, VERSION, FLAG_LEN16 if len16 else 0, V, H, P, int(L), len(joined), nb, len(payload))
    sec = _sections(len16, V, H, nb, len(payload), len(joined))
    img = bytearray(sec["total"])
    img[:len(hdr)] = hdr

    def put(name, data):
        img[sec[name]:sec[name] + len(data)] = data
    put("node_len", node_len.astype("<u2" if len16 else "<u4").tobytes())
    put("path_off", path_off.astype("<u8").tobytes())
    put("blk_first", blk_first.astype("<u4").tobytes())
    put("blk_off", (true_off if blk_off is None else blk_off).astype("<u4").tobytes())
    put("payload", payload)
    put("names", joined)
    put("end", struct.pack("<Q", fnv1a64(hdr)))
    with open(path, "wb") as f:
        f.write(bytes(img))
    return path
