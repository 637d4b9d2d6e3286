"""Host-side mirror of the reference's profiling interface over the C ABI.

Method names follow the reference functions they stand in for (profile.rs / rcls.rs)
so the parity tests read like tests of the reference:
    rcls_profile            rcls.rs:452-458   (+ species counters profile.rs:208-297)
    trio_nodes_info         profile.rs:658-740
    get_node_abundances     profile.rs:743-1026
    strain_profiling        profile.rs:3291-3323 (optimize_otu + abundace_constraint per species)
    pao_solve               the X_opt solver seam, profile.rs:2690-2698
Everything here is plumbing: numpy arrays in, ctypes call, numpy arrays out.
"""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import PantaxHipError, as_c, p


class Engine:
    def __init__(self, device=0):
        self.lib = _ffi.load()
        self.ctx = C.c_void_p()
        dev = (C.c_int * 1)(device)
        rc = self.lib.pantax_hip_init(C.byref(self.ctx), dev, 1)
        if rc != 0:
            raise PantaxHipError(rc, self.lib.pantax_hip_last_error(None).decode())
        self.db = None
        self.reads = None
        self._keep = []
        self._step_buf = None
        self._collect_buf = None
        self._inflight = 0

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc != 0:
            raise PantaxHipError(rc, self.lib.pantax_hip_last_error(self.ctx).decode())

    def close(self):
        if self.ctx:
            if self.reads:
                self.lib.pantax_hip_reads_free(self.ctx, self.reads)
                self.reads = None
            if self.db:
                self.lib.pantax_hip_db_free(self.ctx, self.db)
                self.db = None
            self.lib.pantax_hip_destroy(self.ctx)
            self.ctx = None

    def release(self):
        """free the resident db and reads (HBM), keep the ctx"""
        if self.ctx:
            if self.db and self._inflight:
                self.drain_steps()                                # enqueued steps still read the db and the reads
            if self.reads:
                self.lib.pantax_hip_reads_free(self.ctx, self.reads)
                self.reads = None
            if self.db:
                self.lib.pantax_hip_db_free(self.ctx, self.db)
                self.db = None
            self._inflight = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        self._check(self.lib.pantax_hip_sync(self.ctx))

    def set_option(self, name, value=None):
        """pantax_hip_set_option: a switch of this ctx (common.hpp CtxConfig); value None = its default.  The library reads the
        environment only once, at init."""
        self._check(self.lib.pantax_hip_set_option(self.ctx, name.encode(), None if value is None else str(value).encode()))

    def lad_shape_name(self, n_species, max_columns):
        """pantax_hip_lad_shape_name: "roomy" or "compact", the LDS shape the LAD solver takes for a batch of n_species LPs of at most max_columns columns
        under this ctx's option lad_shape."""
        return self.lib.pantax_hip_lad_shape_name(self.ctx, int(n_species), int(max_columns)).decode()

    # ------------------------------------------------------------------ uploads
    def upload_db(self, species):
        """species: list of objects with node_len, path_off, path_nodes, range_start, range_end
        (synthdata.SpeciesGraph or pantax_amd.io graphs), haplotypes in byte order."""
        if self.db:
            self.lib.pantax_hip_db_free(self.ctx, self.db)
            self.db = None
            self._inflight = 0
        S = len(species)
        self.S = S
        self.range_start = as_c([g.range_start for g in species], np.int64)
        self.range_end = as_c([g.range_end for g in species], np.int64)
        self.node_off = np.zeros(S + 1, dtype=np.uint64)
        self.node_off[1:] = np.cumsum([len(g.node_len) for g in species])
        self.hap_off = np.zeros(S + 1, dtype=np.uint64)
        self.hap_off[1:] = np.cumsum([len(g.path_off) - 1 for g in species])
        self.V = int(self.node_off[-1])
        self.H = int(self.hap_off[-1])
        # one part per species (pantax_hip_db_upload_parts): the arrays travel as they are, nothing is concatenated on the host
        keep = []
        parts = (_ffi.GraphPart * S)()
        for i, g in enumerate(species):
            nl, po, pn = as_c(g.node_len, np.int64), as_c(g.path_off, np.uint64), as_c(g.path_nodes, np.uint32)
            keep.append((nl, po, pn))
            parts[i] = _ffi.GraphPart(len(nl), len(po) - 1, nl.ctypes.data, po.ctypes.data, pn.ctypes.data if len(pn) else None)
        db = C.c_void_p()
        self._check(self.lib.pantax_hip_db_upload_parts(self.ctx, C.c_uint32(S), p(self.range_start), p(self.range_end), parts, C.byref(db)))
        self.db = db
        self.U = None

    def upload_db_flat(self, species):
        """The same db through pantax_hip_db_upload (SURVEY 8b's struct of flat arrays: all species concatenated by the caller)."""
        if self.db:
            self.lib.pantax_hip_db_free(self.ctx, self.db)
            self.db = None
            self._inflight = 0
        S = len(species)
        self.S = S
        self.range_start = as_c([g.range_start for g in species], np.int64)
        self.range_end = as_c([g.range_end for g in species], np.int64)
        self.node_off = np.zeros(S + 1, dtype=np.uint64)
        self.node_off[1:] = np.cumsum([len(g.node_len) for g in species])
        self.hap_off = np.zeros(S + 1, dtype=np.uint64)
        self.hap_off[1:] = np.cumsum([len(g.path_off) - 1 for g in species])
        node_len = as_c(np.concatenate([g.node_len for g in species]), np.int64)
        offs = [np.zeros(1, dtype=np.uint64)]
        base = 0
        for g in species:
            offs.append(np.asarray(g.path_off[1:], dtype=np.uint64) + np.uint64(base))
            base += int(g.path_off[-1])
        path_off = as_c(np.concatenate(offs), np.uint64)
        path_nodes = as_c(np.concatenate([g.path_nodes for g in species]), np.uint32)
        self.V = int(self.node_off[-1])
        self.H = int(self.hap_off[-1])
        gs = _ffi.Graphs(S, p(self.range_start), p(self.range_end), p(self.node_off), p(node_len),
                         p(self.hap_off), p(path_off), p(path_nodes))
        db = C.c_void_p()
        self._check(self.lib.pantax_hip_db_upload(self.ctx, C.byref(gs), C.byref(db)))
        self.db = db
        self.U = None

    def upload_ranges(self, range_start, range_end):
        """A db of species RANGES only (no graphs): what the binning of a slice of reads needs before the reads are routed
        to the owners of their species; the file seam bins against such a db too."""
        if self.db:
            self.lib.pantax_hip_db_free(self.ctx, self.db)
            self.db = None
            self._inflight = 0
        self.range_start = as_c(range_start, np.int64)
        self.range_end = as_c(range_end, np.int64)
        self.S = len(self.range_start)
        self.V = self.H = 0
        gs = _ffi.Graphs(self.S, p(self.range_start), p(self.range_end), None, None, None, None, None)
        db = C.c_void_p()
        self._check(self.lib.pantax_hip_db_upload(self.ctx, C.byref(gs), C.byref(db)))
        self.db = db
        self.U = None

    def upload_reads(self, step_off, node_id, pstart, pend, qlen, mapq, flags=None):
        if self.reads:
            self.lib.pantax_hip_reads_free(self.ctx, self.reads)
            self.reads = None
        for name, a in (("step_off", step_off), ("node_id", node_id), ("pstart", pstart), ("pend", pend), ("qlen", qlen)):
            a = np.asarray(a)
            if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
                raise ValueError("%s outside the packed u32 range [0, 2^32): GAF columns are non-negative" % name)
        arrs = dict(step_off=as_c(step_off, np.uint32), node_id=as_c(node_id, np.uint32), pstart=as_c(pstart, np.uint32),
                    pend=as_c(pend, np.uint32), qlen=as_c(qlen, np.uint32), mapq=as_c(mapq, np.uint8),
                    flags=None if flags is None else as_c(flags, np.uint8))
        R = len(arrs["pstart"])
        self.R = R
        self.T = len(arrs["node_id"])
        pr = _ffi.PackedReads(R, self.T, p(arrs["step_off"]), p(arrs["node_id"]), p(arrs["pstart"]), p(arrs["pend"]),
                              p(arrs["qlen"]), p(arrs["mapq"]), p(arrs["flags"]))
        rd = C.c_void_p()
        self._check(self.lib.pantax_hip_reads_upload(self.ctx, C.byref(pr), C.byref(rd)))
        self.reads = rd

    def upload_packed(self, reads, flags=None):
        """reads: synthdata.PackedReads (int64 host arrays)"""
        mapq = np.where((reads.mapq < 0) | (reads.mapq > 254), 255, reads.mapq)
        self.upload_reads(reads.step_off, reads.node_id, reads.pstart, reads.pend, reads.qlen, mapq, flags)

    def load_reads_from_gaf(self, path, columns=True, ids=False):
        """GAF file -> packed reads resident in HBM, tokenised on the device (pantax_hip_reads_load_gaf).
        -> dict(qlen, mapq, flags) of the host-side columns (columns=False: None, nothing is copied out); the walks stay on
        the device.  ids=True adds the keys of pantax_amd.io.gaf_ids (id hashes and the tokenizer's route; no id spans on this path)."""
        if self.reads:
            self.lib.pantax_hip_reads_free(self.ctx, self.reads)
            self.reads = None
        rd, gaf = C.c_void_p(), C.c_void_p()
        if not columns:   # no gaf handle: the library does not bring the per-read host columns back at all
            self._check(self.lib.pantax_hip_reads_load_gaf(self.ctx, str(path).encode(), C.byref(rd), None))
            self.reads = rd
            self.R = self.T = None       # not known on the host (the counters of a binning pass tell)
            return None
        self._check(self.lib.pantax_hip_reads_load_gaf(self.ctx, str(path).encode(), C.byref(rd), C.byref(gaf)))
        self.reads = rd
        try:
            v = _ffi.PackedReads()
            self.lib.pantax_hip_gaf_view(gaf, C.byref(v))
            self.R = int(v.n_reads)
            arr = lambda ptr, dt: (np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(self.R,)).copy()
                                   if self.R else np.zeros(0, dtype=dt))
            out = dict(qlen=arr(v.qlen, np.uint32), mapq=arr(v.mapq, np.uint8), flags=arr(v.flags, np.uint8))
            if ids:
                from . import io as pio
                out.update(pio.gaf_ids(self.lib, gaf))
            return out
        finally:
            self.lib.pantax_hip_gaf_free(gaf)

    # ------------------------------------------------------------------ reads routed to the owner of their species
    def route_pack(self, owner_of_species, world):
        """The resident reads (binned against the resident db) as one message per owner rank (stable partition on the
        device).  -> (route handle, n_reads_to [W], n_steps_to [W]); free the handle with route_free."""
        own = as_c(owner_of_species, np.int32)
        assert len(own) == self.S
        nr = np.zeros(world, dtype=np.uint64)
        nt = np.zeros(world, dtype=np.uint64)
        rt = C.c_void_p()
        self._check(self.lib.pantax_hip_reads_route_pack(self.ctx, self.db, self.reads, p(own), int(world), C.byref(rt), p(nr), p(nt)))
        return rt, nr, nt

    def route_buffer(self, route, world, on_device=False):
        """-> (address of the W messages back to back, word offsets [W+1]); device pointer when on_device, else pinned host memory."""
        buf = C.c_void_p()
        off = np.zeros(world + 1, dtype=np.uint64)
        self._check(self.lib.pantax_hip_route_buffer(self.ctx, route, int(bool(on_device)), C.byref(buf), p(off)))
        return buf.value or 0, off

    def route_messages(self, route, world):
        """host copies of the W messages (uint32 arrays)"""
        addr, off = self.route_buffer(route, world, on_device=False)
        n = int(off[-1])
        if n == 0:
            return [np.zeros(0, dtype=np.uint32) for _ in range(world)]
        whole = np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_uint32)), shape=(n,))
        return [whole[int(off[d]):int(off[d + 1])].copy() for d in range(world)]

    def route_free(self, route):
        self.lib.pantax_hip_route_free(self.ctx, route)

    def reads_from_routed(self, recv, n_reads_from, n_steps_from, on_device=False):
        """recv: the messages of ranks 0..W-1 for this rank back to back -- a uint32 numpy array (host) or, with on_device, the
        integer address of device memory.  Replaces the resident reads."""
        if self.reads:
            self.lib.pantax_hip_reads_free(self.ctx, self.reads)
            self.reads = None
        nr = as_c(n_reads_from, np.uint64)
        nt = as_c(n_steps_from, np.uint64)
        if on_device:
            ptr = C.c_void_p(int(recv))
        else:
            recv = as_c(recv, np.uint32)
            ptr = p(recv)
        rd = C.c_void_p()
        self._check(self.lib.pantax_hip_reads_from_routed(self.ctx, ptr, int(bool(on_device)), len(nr), p(nr), p(nt), C.byref(rd)))
        self.reads = rd
        self.R = int(nr.sum())
        self.T = int(nt.sum())

    def set_read_flags(self, flags):
        f = None if flags is None else as_c(flags, np.uint8)
        self._check(self.lib.pantax_hip_reads_set_flags(self.ctx, self.reads, p(f)))

    # ------------------------------------------------------------------ stages
    def rcls_profile(self, want_species=True):
        """-> (species_idx [R] int32 or None, read_count, base_sum, less_multi, uniq_count [S] int64)"""
        sp = np.empty(self.R, dtype=np.int32) if want_species else None
        outs = [np.zeros(self.S, dtype=np.int64) for _ in range(4)]
        self._check(self.lib.pantax_hip_bin_reads(self.ctx, self.db, self.reads, p(sp), *[p(o) for o in outs]))
        return (sp, *outs)

    def species_profiling(self, counts, avg_len, filtered=True):
        """profile.rs:299-349 finishing -> keep [S] uint8, predicted_coverage [S], predicted_abundance [S]"""
        rc, bs, lm, uq = [as_c(c, np.int64) for c in counts]
        avg = as_c(avg_len, np.float64)
        keep = np.zeros(self.S, dtype=np.uint8)
        absolute = np.zeros(self.S)
        abundance = np.zeros(self.S)
        self._check(self.lib.pantax_hip_species_profile(self.ctx, self.db, self.reads, p(rc), p(bs), p(lm), p(uq), p(avg),
                                                        int(filtered), p(keep), p(absolute), p(abundance)))
        return keep, absolute, abundance

    def db_reset(self):
        self._check(self.lib.pantax_hip_db_reset(self.ctx, self.db))
        self.U = None

    def abundance_filter(self, met, species_reported=None, single_cov_diff=0.2, min_cov=0):
        """abundance_est filters (profile.rs:3219-3245) -> pass [H] uint8, per-species sum_all [S], sum_pass [S]"""
        rep = None if species_reported is None else as_c(species_reported, np.uint8)
        passed = np.zeros(max(self.H, 1), dtype=np.uint8)
        sa = C.c_double(0)
        sp = C.c_double(0)
        s_all = np.zeros(self.S)
        s_pass = np.zeros(self.S)
        rc = self.lib.pantax_hip_abundance_filter(C.c_uint32(self.S), p(self.hap_off), met, p(rep), C.c_double(single_cov_diff),
                                                  C.c_int64(min_cov), p(passed), C.byref(sa), C.byref(sp), p(s_all), p(s_pass))
        self._check(rc)
        return passed[: self.H], s_all, s_pass

    def read_strains(self, cand_off, cand_hap, cand_w, fill=None):
        """Per-read strain assignment (pantax_hip_read_strains) of the resident reads, binned against the resident db.
        cand_off [S+1], cand_hap (species-local haplotype indices), cand_w (weights) -> (hap uint32, n int32, posterior float64), [R] each in file
        order.  Only reads binned to a species of the db are written; every other entry keeps its value from `fill` ((hap, n, post) arrays),
        by default (0xFFFFFFFF, -2, 0.0)."""
        if self.R is None:
            raise ValueError("read_strains: the number of reads is not known on the host (load_reads_from_gaf(columns=True))")
        co = as_c(cand_off, np.uint64)
        ch = as_c(cand_hap, np.uint32)
        cw = as_c(cand_w, np.float64)
        if len(co) != self.S + 1 or len(ch) != int(co[-1]) or len(cw) != len(ch):
            raise ValueError("read_strains: cand_off needs S + 1 entries and cand_hap / cand_w cand_off[-1] each")
        if fill is None:
            hap = np.full(self.R, 0xFFFFFFFF, dtype=np.uint32)
            n = np.full(self.R, -2, dtype=np.int32)
            post = np.zeros(self.R)
        else:
            hap, n, post = as_c(fill[0], np.uint32).copy(), as_c(fill[1], np.int32).copy(), as_c(fill[2], np.float64).copy()
        cs = _ffi.ReadStrainSet(self.S, co.ctypes.data, ch.ctypes.data if len(ch) else None, cw.ctypes.data if len(cw) else None)
        self._check(self.lib.pantax_hip_read_strains(self.ctx, self.db, self.reads, C.byref(cs), p(hap), p(n), p(post)))
        return hap, n, post

    def strain_read_support(self, cand_off, cand_hap, cand_w):
        """Per-strain read support (pantax_hip_strain_read_support) of the resident reads, binned against the resident db.  The candidate set of
        read_strains -> (hap uint64 [C, 3, 3]: compatible / unique / assigned of every candidate entry, species uint64 [S, 4, 3]: counted / unexplained /
        ambiguous / uninformative, pair_off uint64 [S+1], pair uint64 [pair_off[-1]]: the K_s x K_s shared-read counts of every species of K_s <= 64);
        the last axis of hap and species is {n_reads, n_steps, span}."""
        co = as_c(cand_off, np.uint64)
        ch = as_c(cand_hap, np.uint32)
        cw = as_c(cand_w, np.float64)
        if len(co) != self.S + 1 or len(ch) != int(co[-1]) or len(cw) != len(ch):
            raise ValueError("strain_read_support: cand_off needs S + 1 entries and cand_hap / cand_w cand_off[-1] each")
        cs = _ffi.ReadStrainSet(self.S, co.ctypes.data, ch.ctypes.data if len(ch) else None, cw.ctypes.data if len(cw) else None)
        hap = np.zeros((len(ch), 3, 3), dtype=np.uint64)
        species = np.zeros((self.S, 4, 3), dtype=np.uint64)
        pair_off = np.zeros(self.S + 1, dtype=np.uint64)
        k = np.diff(co.astype(np.int64))
        pair = np.zeros(int((k[k <= 64] ** 2).sum()), dtype=np.uint64)
        self._check(self.lib.pantax_hip_strain_read_support(self.ctx, self.db, self.reads, C.byref(cs), p(hap) if len(ch) else None,
                                                            p(species) if self.S else None, p(pair_off), len(pair), p(pair) if len(pair) else None))
        return hap, species, pair_off, pair

    def fragment_mates(self, key, tag):
        """pantax_hip_fragment_mates: the mate of every read from its fragment key and tag (fragment_key) -> (mate uint32 [n]: the index of the mate,
        MATE_NONE or MATE_AMBIGUOUS; counts uint64 [4]: pairs, reads without a mate, ambiguous reads, keys seen three times or more)."""
        k = as_c(key, np.uint64)
        t = as_c(tag, np.uint8)
        if len(k) != len(t):
            raise ValueError("fragment_mates: key and tag are of one length")
        mate = np.full(len(k), _ffi.MATE_NONE, dtype=np.uint32)
        counts = np.zeros(4, dtype=np.uint64)
        q = lambda a: p(a) if a.size else None
        self._check(self.lib.pantax_hip_fragment_mates(self.ctx, len(k), q(k), q(t), q(mate), p(counts)))
        return mate, counts

    def strain_fragments(self, cand_off, cand_hap, cand_w, mate, want_n=False, fill=None, pair_cap=None):
        """Fragment support (pantax_hip_strain_fragments) of the resident reads, binned against the resident db: read pairs as the unit of strain
        compatibility.  The candidate set of read_strains and mate uint32 [R] in file order (fragment_mates) -> (hap uint64 [C, 4, 3]: compatible /
        unique / unique_by_pair / assigned of every candidate entry, species uint64 [S, 9, 3]: counted / paired / concordant / discordant / half /
        unexplained / single / multi / mate_elsewhere, status int32 [S], pair_off uint64 [S+1], pair uint64 [pair_off[-1]]: the K_s x K_s discordant
        fragment counts of every species of K_s <= 64, frag_n int32 [R] or None); the last axis of hap and species is {n, n_steps, span}.  want_n: |F| of
        every read of a paired fragment of a served species, -1 for the other reads binned to the db; entries of other reads keep `fill` (default -2).
        pair_cap None: sized inside; a number that is too small raises PantaxHipError with code E_LIMIT."""
        co = as_c(cand_off, np.uint64)
        ch = as_c(cand_hap, np.uint32)
        cw = as_c(cand_w, np.float64)
        mt = as_c(mate, np.uint32)
        if len(co) != self.S + 1 or len(ch) != int(co[-1]) or len(cw) != len(ch):
            raise ValueError("strain_fragments: cand_off needs S + 1 entries and cand_hap / cand_w cand_off[-1] each")
        if self.R is None or len(mt) != self.R:
            raise ValueError("strain_fragments: mate needs one entry per resident read")
        cs = _ffi.ReadStrainSet(self.S, co.ctypes.data, ch.ctypes.data if len(ch) else None, cw.ctypes.data if len(cw) else None)
        hap = np.zeros((len(ch), 4, 3), dtype=np.uint64)
        species = np.zeros((self.S, _ffi.FRAGMENT_CLASSES, 3), dtype=np.uint64)
        status = np.zeros(self.S, dtype=np.int32)
        pair_off = np.zeros(self.S + 1, dtype=np.uint64)
        k = np.diff(co.astype(np.int64))
        pair = np.zeros(int((k[k <= 64] ** 2).sum()) if pair_cap is None else int(pair_cap), dtype=np.uint64)
        n = None
        if want_n:
            n = np.full(self.R, -2, dtype=np.int32) if fill is None else as_c(fill, np.int32).copy()
        q = lambda a: p(a) if a is not None and a.size else None
        self._check(self.lib.pantax_hip_strain_fragments(self.ctx, self.db, self.reads, C.byref(cs), q(mt), q(hap), q(species), q(status), p(pair_off),
                                                         len(pair), q(pair), q(n)))
        return hap, species, status, pair_off, pair, n

    def strain_mosaic(self, cand_off, cand_hap, cand_w, junction_cap=None):
        """Mosaic reads (pantax_hip_strain_mosaic) of the resident reads, binned against the resident db: every counted read of a species of 1 .. 64
        candidates cut into the fewest stretches that each fit one candidate.  The candidate set of read_strains -> (species uint64 [S, 6, 3]: counted /
        compatible / mosaic1 / mosaic2 / mosaic3plus / foreign, extra uint64 [S, 3]: n_segments / n_breaks / foreign_steps, hap uint64 [C, 2]: segments /
        steps of every candidate entry, pair_off uint64 [S+1], pair uint64 [pair_off[-1]]: the K_s x K_s switch counts [left][right], junction uint32
        [J, 3]: species / node_a / node_b (species-local) in ascending order, junction_count uint64 [J], n_breaks_total); the last axis of species is
        {n_reads, n_steps, span}.  junction_cap None: sized inside (a second call when the first guess is short); 0: junctions are not collected; a
        number that is too small raises PantaxHipError with code E_LIMIT."""
        co = as_c(cand_off, np.uint64)
        ch = as_c(cand_hap, np.uint32)
        cw = as_c(cand_w, np.float64)
        if len(co) != self.S + 1 or len(ch) != int(co[-1]) or len(cw) != len(ch):
            raise ValueError("strain_mosaic: cand_off needs S + 1 entries and cand_hap / cand_w cand_off[-1] each")
        cs = _ffi.ReadStrainSet(self.S, co.ctypes.data, ch.ctypes.data if len(ch) else None, cw.ctypes.data if len(cw) else None)
        species = np.zeros((self.S, _ffi.MOSAIC_CLASSES, 3), dtype=np.uint64)
        extra = np.zeros((self.S, 3), dtype=np.uint64)
        hap = np.zeros((len(ch), 2), dtype=np.uint64)
        pair_off = np.zeros(self.S + 1, dtype=np.uint64)
        k = np.diff(co.astype(np.int64))
        pair = np.zeros(int((k[k <= 64] ** 2).sum()), dtype=np.uint64)
        q = lambda a: p(a) if len(a) else None
        cap = 1024 if junction_cap is None else int(junction_cap)
        while True:
            jn = np.zeros((cap, 3), dtype=np.uint32)
            jc = np.zeros(cap, dtype=np.uint64)
            n_j, n_b = C.c_uint64(0), C.c_uint64(0)
            rc = self.lib.pantax_hip_strain_mosaic(self.ctx, self.db, self.reads, C.byref(cs), q(species), q(extra), q(hap), p(pair_off), len(pair), q(pair),
                                                   cap, q(jn), q(jc), C.byref(n_j), C.byref(n_b))
            if rc == _ffi.E_LIMIT and junction_cap is None and cap and int(n_b.value) > cap:
                cap = int(n_b.value)
                continue
            self._check(rc)
            break
        n = int(n_j.value)
        return species, extra, hap, pair_off, pair, jn[:n].copy(), jc[:n].copy(), int(n_b.value)

    def strain_read_em(self, cand_off, cand_hap, cand_len, max_iter=1000, tol=1e-6):
        """Read classes and the read-based estimate (pantax_hip_strain_read_em) of the resident reads, binned against the resident db.  The candidate set
        of read_strains with cand_len (uint64 graph bases of every candidate) in place of the weights -> (species uint64 [S, 2, 3]: counted /
        unexplained, cls_off uint64 [S+1], cls_mask uint64 [J], cls_q uint64 [J, 3]: the classes of every species of 1 .. 64 candidates in ascending
        mask, bit i = the candidate with the i-th smallest haplotype index, x float64 [C] in the caller's order, n_iter uint32 [S], converged int32 [S],
        delta float64 [S]); the last axis of species and cls_q is {n_reads, n_steps, span}."""
        co = as_c(cand_off, np.uint64)
        ch = as_c(cand_hap, np.uint32)
        cl = as_c(cand_len, np.uint64)
        if len(co) != self.S + 1 or len(ch) != int(co[-1]) or len(cl) != len(ch):
            raise ValueError("strain_read_em: cand_off needs S + 1 entries and cand_hap / cand_len cand_off[-1] each")
        cs = _ffi.ReadEmSet(self.S, co.ctypes.data, ch.ctypes.data if len(ch) else None, cl.ctypes.data if len(cl) else None, int(max_iter), float(tol))
        species = np.zeros((self.S, 2, 3), dtype=np.uint64)
        cls_off = np.zeros(self.S + 1, dtype=np.uint64)
        x = np.zeros(len(ch), dtype=np.float64)
        n_iter = np.zeros(self.S, dtype=np.uint32)
        converged = np.zeros(self.S, dtype=np.int32)
        delta = np.zeros(self.S, dtype=np.float64)
        cap = 4096
        while True:   # a second call only when a species set has more classes than the first guess holds: cls_off then says how many
            cls_mask = np.zeros(cap, dtype=np.uint64)
            cls_q = np.zeros((cap, 3), dtype=np.uint64)
            rc = self.lib.pantax_hip_strain_read_em(self.ctx, self.db, self.reads, C.byref(cs), p(species) if self.S else None, p(cls_off), cap, p(cls_mask),
                                                    p(cls_q), p(x) if len(ch) else None, p(n_iter) if self.S else None,
                                                    p(converged) if self.S else None, p(delta) if self.S else None)
            if rc == _ffi.E_LIMIT and int(cls_off[-1]) > cap:
                cap = int(cls_off[-1])
                continue
            self._check(rc)
            break
        n = int(cls_off[-1])
        return species, cls_off, cls_mask[:n].copy(), cls_q[:n].copy(), x, n_iter, converged, delta

    def strain_cov_track(self, sel_off, sel_hap, window):
        """Per-strain windowed coverage track (pantax_hip_strain_cov_track) of the coverage result get_node_abundances left on the device.
        sel_off [S+1], sel_hap (species-local haplotype indices, no repeats within a species), window W >= 1 in bases ->
        (win_off uint64 [C+1], n_nodes uint32, len, covered, bases uint64): the windows of selection entry c are [win_off[c], win_off[c+1])."""
        so = as_c(sel_off, np.uint64)
        sh = as_c(sel_hap, np.uint32)
        if len(so) != self.S + 1 or len(sh) != int(so[-1]):
            raise ValueError("strain_cov_track: sel_off needs S + 1 entries and sel_hap sel_off[-1]")
        cs = _ffi.CovTrackSet(self.S, so.ctypes.data, sh.ctypes.data if len(sh) else None, int(window))
        win_off = np.zeros(len(sh) + 1, dtype=np.uint64)
        rc = self.lib.pantax_hip_strain_cov_track(self.ctx, self.db, C.byref(cs), p(win_off), 0, None, None, None, None)   # sizes the arrays
        if rc != _ffi.E_LIMIT:
            self._check(rc)
        n = int(win_off[-1])
        n_nodes = np.zeros(n, dtype=np.uint32)
        ln, covered, bases = (np.zeros(n, dtype=np.uint64) for _ in range(3))
        if n:
            self._check(self.lib.pantax_hip_strain_cov_track(self.ctx, self.db, C.byref(cs), p(win_off), n, p(n_nodes), p(ln), p(covered), p(bases)))
        return win_off, n_nodes, ln, covered, bases

    def strain_growth(self, sel_off, sel_hap, window):
        """Own-node windows along selected haplotypes (pantax_hip_strain_growth) of the coverage result get_node_abundances left on the device: the input
        of growth_fit.  sel_off [S+1], sel_hap (species-local haplotype indices, no repeats within a species), window W >= 1 in bases ->
        (win_off uint64 [C+1], n_own uint32, len, len_own, bases_own uint64): the windows of selection entry c are [win_off[c], win_off[c+1]); a step is
        own when no other selected haplotype of its species walks its node."""
        so = as_c(sel_off, np.uint64)
        sh = as_c(sel_hap, np.uint32)
        if len(so) != self.S + 1 or len(sh) != int(so[-1]):
            raise ValueError("strain_growth: sel_off needs S + 1 entries and sel_hap sel_off[-1]")
        cs = _ffi.CovTrackSet(self.S, so.ctypes.data, sh.ctypes.data if len(sh) else None, int(window))
        win_off = np.zeros(len(sh) + 1, dtype=np.uint64)
        rc = self.lib.pantax_hip_strain_growth(self.ctx, self.db, C.byref(cs), p(win_off), 0, None, None, None, None)   # sizes the arrays
        if rc != _ffi.E_LIMIT:
            self._check(rc)
        n = int(win_off[-1])
        n_own = np.zeros(n, dtype=np.uint32)
        ln, len_own, bases_own = (np.zeros(n, dtype=np.uint64) for _ in range(3))
        if n:
            self._check(self.lib.pantax_hip_strain_growth(self.ctx, self.db, C.byref(cs), p(win_off), n, p(n_own), p(ln), p(len_own), p(bases_own)))
        return win_off, n_own, ln, len_own, bases_own

    def strain_segments(self, sel_off, sel_hap, peak_depth, min_len):
        """Absent and amplified segments along selected haplotypes (pantax_hip_strain_segments) of the coverage result get_node_abundances left on the
        device.  sel_off [S+1], sel_hap (species-local haplotype indices, no repeats within a species), peak_depth (one uint64 per entry, or one number
        for all; 0: no peak class), min_len >= 1 in bases -> (seg_off uint64 [C+1], hap_len uint64 [C], n_runs, run_len, run_max uint64 [C, 2]: gap /
        peak over all runs, seg_class uint8, seg_step uint64, seg_n_steps uint32, seg_start, seg_len, seg_bases uint64): the segments of at least
        min_len bases of selection entry c are [seg_off[c], seg_off[c+1]), in ascending start."""
        so = as_c(sel_off, np.uint64)
        sh = as_c(sel_hap, np.uint32)
        if len(so) != self.S + 1 or len(sh) != int(so[-1]):
            raise ValueError("strain_segments: sel_off needs S + 1 entries and sel_hap sel_off[-1]")
        pd = as_c(np.broadcast_to(np.asarray(peak_depth, dtype=np.uint64), (len(sh),)), np.uint64)
        cs = _ffi.SegmentSet(self.S, so.ctypes.data, sh.ctypes.data if len(sh) else None, pd.ctypes.data if len(sh) else None, int(min_len))
        seg_off = np.zeros(len(sh) + 1, dtype=np.uint64)
        hap_len = np.zeros(len(sh), dtype=np.uint64)
        n_runs, run_len, run_max = (np.zeros((len(sh), 2), dtype=np.uint64) for _ in range(3))
        q = lambda a: p(a) if len(a) else None
        rc = self.lib.pantax_hip_strain_segments(self.ctx, self.db, C.byref(cs), p(seg_off), 0, q(hap_len), q(n_runs), q(run_len), q(run_max),
                                                 None, None, None, None, None, None)   # sizes the arrays
        if rc != _ffi.E_LIMIT:
            self._check(rc)
        n = int(seg_off[-1])
        cls = np.zeros(n, dtype=np.uint8)
        n_steps = np.zeros(n, dtype=np.uint32)
        step, start, ln, bases = (np.zeros(n, dtype=np.uint64) for _ in range(4))
        if n:
            self._check(self.lib.pantax_hip_strain_segments(self.ctx, self.db, C.byref(cs), p(seg_off), n, q(hap_len), q(n_runs), q(run_len), q(run_max),
                                                            p(cls), p(step), p(n_steps), p(start), p(ln), p(bases)))
        return seg_off, hap_len, n_runs, run_len, run_max, cls, step, n_steps, start, ln, bases

    def strain_evidence(self, sel_off, sel_hap):
        """Per-strain node evidence (pantax_hip_strain_evidence) of the coverage result get_node_abundances left on the device.
        sel_off [S+1], sel_hap (species-local haplotype indices, no repeats within a species) -> (hap uint64 [C, 2, 4]: all / private of every
        selection entry, species uint64 [S, 3, 4]: total / orphan / core), the last axis {n_nodes, len, covered, bases}."""
        so = as_c(sel_off, np.uint64)
        sh = as_c(sel_hap, np.uint32)
        if len(so) != self.S + 1 or len(sh) != int(so[-1]):
            raise ValueError("strain_evidence: sel_off needs S + 1 entries and sel_hap sel_off[-1]")
        cs = _ffi.EvidenceSet(self.S, so.ctypes.data, sh.ctypes.data if len(sh) else None)
        hap = np.zeros((len(sh), 2, 4), dtype=np.uint64)
        species = np.zeros((self.S, 3, 4), dtype=np.uint64)
        self._check(self.lib.pantax_hip_strain_evidence(self.ctx, self.db, C.byref(cs), p(hap) if len(sh) else None, p(species) if self.S else None))
        return hap, species

    def strain_fit(self, sel_off, sel_hap, sel_w):
        """Model fit per strain (pantax_hip_strain_fit) of the coverage result get_node_abundances left on the device.  sel_off [S+1], sel_hap as for
        strain_evidence, sel_w float64 [C]: the predicted coverage of every selection entry (finite, >= 0) -> (hap uint64 [C, 2, 8]: all / private of
        every selection entry, species uint64 [S, 3, 8]: total / explained / orphan), the last axis {n_nodes, len, bases, expected, excess, deficit,
        blind_nodes, blind_expected}."""
        so = as_c(sel_off, np.uint64)
        sh = as_c(sel_hap, np.uint32)
        sw = as_c(sel_w, np.float64)
        if len(so) != self.S + 1 or len(sh) != int(so[-1]) or len(sw) != len(sh):
            raise ValueError("strain_fit: sel_off needs S + 1 entries, sel_hap and sel_w sel_off[-1]")
        cs = _ffi.FitSet(self.S, so.ctypes.data, sh.ctypes.data if len(sh) else None, sw.ctypes.data if len(sh) else None)
        hap = np.zeros((len(sh), 2, 8), dtype=np.uint64)
        species = np.zeros((self.S, 3, 8), dtype=np.uint64)
        self._check(self.lib.pantax_hip_strain_fit(self.ctx, self.db, C.byref(cs), p(hap) if len(sh) else None, p(species) if self.S else None))
        return hap, species

    def strain_bootstrap(self, sel_off, sel_hap, sp_key, seed=42, n_replicates=100):
        """Bootstrap of the strain fit (pantax_hip_strain_bootstrap) on the coverage result get_node_abundances left on the device.  sel_off [S+1], sel_hap as
        for strain_evidence (entry c of species s is column c - sel_off[s] of its LP), sp_key uint64 [S]: the species' key of the weight hash -> (x float64
        [R, C], obj float64 [R, S], rows uint64 [R, S], status int32 [R, S]) with R = n_replicates + 1; replicate 0 is the plain refit."""
        so = as_c(sel_off, np.uint64)
        sh = as_c(sel_hap, np.uint32)
        sk = as_c(sp_key, np.uint64)
        if len(so) != self.S + 1 or len(sh) != int(so[-1]) or len(sk) != self.S:
            raise ValueError("strain_bootstrap: sel_off needs S + 1 entries, sel_hap sel_off[-1], sp_key S")
        R = int(n_replicates) + 1
        cs = _ffi.BootstrapSet(self.S, so.ctypes.data, sh.ctypes.data if len(sh) else None, sk.ctypes.data if self.S else None, int(seed), int(n_replicates))
        x = np.zeros((R, len(sh)), dtype=np.float64)
        obj = np.zeros((R, self.S), dtype=np.float64)
        rows = np.zeros((R, self.S), dtype=np.uint64)
        status = np.zeros((R, self.S), dtype=np.int32)
        self._check(self.lib.pantax_hip_strain_bootstrap(self.ctx, self.db, C.byref(cs), p(x) if len(sh) else None, p(obj) if self.S else None,
                                                         p(rows) if self.S else None, p(status) if self.S else None))
        return x, obj, rows, status

    def strain_dropout(self, sel_off, sel_hap):
        """Leave-one-out test of the strain fit (pantax_hip_strain_dropout) on the coverage result get_node_abundances left on the device.  sel_off [S+1],
        sel_hap as for strain_bootstrap.  Species s of K_s columns has K_s + 1 entries: 0 the plain refit, k + 1 the fit without column k; entry (s, e) is
        q = sel_off[s] + s + e -> (x: list of S float64 [K_s + 1, K_s] blocks (views of one array, x[0].base), obj float64 [Q], status int32 [Q],
        rows uint64 [S], count uint64 [Q, 4] = n_member, n_only, n_worse, n_better) with Q = sel_off[-1] + S."""
        so = as_c(sel_off, np.uint64)
        sh = as_c(sel_hap, np.uint32)
        if len(so) != self.S + 1 or len(sh) != int(so[-1]):
            raise ValueError("strain_dropout: sel_off needs S + 1 entries and sel_hap sel_off[-1]")
        K = np.diff(so.astype(np.int64))
        x_off = np.concatenate([[0], np.cumsum((K + 1) * K)]).astype(np.int64)
        Q = len(sh) + self.S
        cs = _ffi.EvidenceSet(self.S, so.ctypes.data, sh.ctypes.data if len(sh) else None)
        flat = np.zeros(max(int(x_off[-1]), 1), dtype=np.float64)
        obj = np.zeros(Q, dtype=np.float64)
        status = np.zeros(Q, dtype=np.int32)
        rows = np.zeros(self.S, dtype=np.uint64)
        count = np.zeros((Q, 4), dtype=np.uint64)
        self._check(self.lib.pantax_hip_strain_dropout(self.ctx, self.db, C.byref(cs), p(flat), p(obj) if self.S else None, p(status) if self.S else None,
                                                       p(rows) if self.S else None, p(count) if self.S else None))
        flat = flat[:int(x_off[-1])]
        x = [flat[int(x_off[s]):int(x_off[s + 1])].reshape(int(K[s]) + 1, int(K[s])) for s in range(self.S)]
        return x, obj, status, rows, count

    def strain_depth(self, sel_off, sel_hap, species=True):
        """Per-strain depth distribution (pantax_hip_strain_depth) of the coverage result get_node_abundances left on the device.
        sel_off [S+1], sel_hap as for strain_evidence -> (hap uint64 [C, 2, 96, 2]: the histograms all / private of every selection entry,
        species uint64 [S, 2, 96, 2]: total / orphan), per bin of depth_bin {n_nodes, len}.  species=False: the species histograms are not
        computed (species_out = NULL) and None is returned in their place."""
        so = as_c(sel_off, np.uint64)
        sh = as_c(sel_hap, np.uint32)
        if len(so) != self.S + 1 or len(sh) != int(so[-1]):
            raise ValueError("strain_depth: sel_off needs S + 1 entries and sel_hap sel_off[-1]")
        cs = _ffi.EvidenceSet(self.S, so.ctypes.data, sh.ctypes.data if len(sh) else None)
        hap = np.zeros((len(sh), 2, _ffi.DEPTH_BINS, 2), dtype=np.uint64)
        sp = np.zeros((self.S, 2, _ffi.DEPTH_BINS, 2), dtype=np.uint64) if species else None
        self._check(self.lib.pantax_hip_strain_depth(self.ctx, self.db, C.byref(cs), p(hap) if len(sh) else None, p(sp) if species and self.S else None))
        return hap, sp

    def strain_near_miss(self, sel_off, sel_hap, cand_off, cand_hap):
        """Unreported-strain near misses (pantax_hip_strain_near_miss) of the coverage result get_node_abundances left on the device.
        sel_off [S+1], sel_hap: the reported haplotypes of every species; cand_off [S+1], cand_hap: the candidates (species-local indices, disjoint from
        the reported ones) -> (cand uint64 [J, 2, 4]: novel / exclusive of every candidate entry, species uint64 [S, 3, 4]: orphan / claimed /
        contested), each {n_nodes, len, covered, bases}."""
        so, sh = as_c(sel_off, np.uint64), as_c(sel_hap, np.uint32)
        co, ch = as_c(cand_off, np.uint64), as_c(cand_hap, np.uint32)
        if len(so) != self.S + 1 or len(sh) != int(so[-1]) or len(co) != self.S + 1 or len(ch) != int(co[-1]):
            raise ValueError("strain_near_miss: sel_off / cand_off need S + 1 entries, sel_hap sel_off[-1] and cand_hap cand_off[-1]")
        cs = _ffi.NearMissSet(self.S, so.ctypes.data, sh.ctypes.data if len(sh) else None, co.ctypes.data, ch.ctypes.data if len(ch) else None)
        cand = np.zeros((len(ch), 2, 4), dtype=np.uint64)
        species = np.zeros((self.S, 3, 4), dtype=np.uint64)
        self._check(self.lib.pantax_hip_strain_near_miss(self.ctx, self.db, C.byref(cs), p(cand) if len(ch) else None, p(species) if self.S else None))
        return cand, species

    def strain_read_rescue(self, sel_off, sel_hap, cand_off, cand_hap):
        """Read rescue (pantax_hip_strain_read_rescue) of the resident reads, binned against the resident db: for every read that fits no reported strain,
        whether a single candidate walks all of its nodes.  sel_off / sel_hap and cand_off / cand_hap as for strain_near_miss; a species of K_s + J_s > 64
        is skipped (counted only) -> (species uint64 [S, 9, 3]: counted / compatible / foreign / foreign_rescued / foreign_patchwork / foreign_novel /
        mosaic / mosaic_rescued / contested, step uint64 [S, 3]: foreign_steps / claimed_steps / novel_steps, cand uint64 [J, 3, 3]: rescued / alone /
        from_foreign of every candidate entry, cand_steps uint64 [J]); the last axis of species and cand is {n_reads, n_steps, span}."""
        so, sh = as_c(sel_off, np.uint64), as_c(sel_hap, np.uint32)
        co, ch = as_c(cand_off, np.uint64), as_c(cand_hap, np.uint32)
        if len(so) != self.S + 1 or len(sh) != int(so[-1]) or len(co) != self.S + 1 or len(ch) != int(co[-1]):
            raise ValueError("strain_read_rescue: sel_off / cand_off need S + 1 entries, sel_hap sel_off[-1] and cand_hap cand_off[-1]")
        cs = _ffi.NearMissSet(self.S, so.ctypes.data, sh.ctypes.data if len(sh) else None, co.ctypes.data, ch.ctypes.data if len(ch) else None)
        species = np.zeros((self.S, _ffi.RESCUE_CLASSES, 3), dtype=np.uint64)
        step = np.zeros((self.S, 3), dtype=np.uint64)
        cand = np.zeros((len(ch), 3, 3), dtype=np.uint64)
        cand_steps = np.zeros(len(ch), dtype=np.uint64)
        self._check(self.lib.pantax_hip_strain_read_rescue(self.ctx, self.db, self.reads, C.byref(cs), p(species) if self.S else None, p(step) if self.S else None,
                                                           p(cand) if len(ch) else None, p(cand_steps) if len(ch) else None))
        return species, step, cand, cand_steps

    def strain_links(self, sel_off, sel_hap):
        """Link support (pantax_hip_strain_links) of the resident reads, binned against the resident db, on the coverage result get_node_abundances left on
        the device: which adjacencies of the selected haplotypes the reads cross.  sel_off [S+1], sel_hap (species-local haplotype indices, no repeats
        within a species; bit p of a link mask = position p of the species' list); a species of K_s > 64 is skipped -> (species uint64 [S, 6]: counted_reads /
        crossings / known / skip / switch / foreign, link uint64 [S, 4]: distinct / distinct crossed / core / core crossed, hap uint64 [C, 8]: links /
        crossed / open / broken / private / private_crossed / private_broken / support, brk_off uint64 [C+1], brk_step, brk_start uint64, brk_node_a,
        brk_node_b uint32 (species-local, in walk order), brk_flank, brk_mask uint64): the break records of entry c are [brk_off[c], brk_off[c+1]), in
        ascending step.  Makes the two calls of the cap protocol."""
        so, sh = as_c(sel_off, np.uint64), as_c(sel_hap, np.uint32)
        if len(so) != self.S + 1 or len(sh) != int(so[-1]):
            raise ValueError("strain_links: sel_off needs S + 1 entries and sel_hap sel_off[-1]")
        cs = _ffi.ReadStrainSet(self.S, so.ctypes.data, sh.ctypes.data if len(sh) else None, None)
        species = np.zeros((self.S, _ffi.LINK_SPECIES_N), dtype=np.uint64)
        link = np.zeros((self.S, 4), dtype=np.uint64)
        hap = np.zeros((len(sh), _ffi.LINK_HAP_N), dtype=np.uint64)
        brk_off = np.zeros(len(sh) + 1, dtype=np.uint64)
        q = lambda a: p(a) if a.size else None
        rc = self.lib.pantax_hip_strain_links(self.ctx, self.db, self.reads, C.byref(cs), q(species), q(link), q(hap), p(brk_off), 0,
                                              None, None, None, None, None, None)   # sizes the arrays
        if rc != _ffi.E_LIMIT:
            self._check(rc)
        n = int(brk_off[-1])
        step, start, flank, mask = (np.zeros(n, dtype=np.uint64) for _ in range(4))
        node_a, node_b = (np.zeros(n, dtype=np.uint32) for _ in range(2))
        if n:
            self._check(self.lib.pantax_hip_strain_links(self.ctx, self.db, self.reads, C.byref(cs), q(species), q(link), q(hap), p(brk_off), n,
                                                         p(step), p(start), p(node_a), p(node_b), p(flank), p(mask)))
        return species, link, hap, brk_off, step, start, node_a, node_b, flank, mask

    def strain_rarefy(self, sel_off, sel_hap, seed=42, n_levels=5, n_replicates=5):
        """Rarefaction of the strain fit (pantax_hip_strain_rarefy) of the resident reads, binned against the resident db, on the coverage result
        get_node_abundances left on the device: the LP of strain_bootstrap refitted on nested subsamples of the reads.  sel_off [S+1], sel_hap as for
        strain_bootstrap.  E = 1 + n_replicates * n_levels entries: 0 the full sample, 1 + (b - 1) n_levels + (l - 1) level l (reads kept with probability
        2^-l) of replicate b -> (x float64 [E, C], obj float64 [E, S], rows uint64 [E, S], status int32 [E, S], reads uint64 [E, S, 2] = counted reads /
        bases added, member uint64 [E, C, 2] = n_member / n_only)."""
        so, sh = as_c(sel_off, np.uint64), as_c(sel_hap, np.uint32)
        if len(so) != self.S + 1 or len(sh) != int(so[-1]):
            raise ValueError("strain_rarefy: sel_off needs S + 1 entries and sel_hap sel_off[-1]")
        E = 1 + max(int(n_replicates), 0) * max(int(n_levels), 0)
        cs = _ffi.RarefySet(self.S, so.ctypes.data, sh.ctypes.data if len(sh) else None, int(seed), int(n_levels), int(n_replicates))
        x = np.zeros((E, len(sh)), dtype=np.float64)
        obj = np.zeros((E, self.S), dtype=np.float64)
        rows = np.zeros((E, self.S), dtype=np.uint64)
        status = np.zeros((E, self.S), dtype=np.int32)
        reads = np.zeros((E, self.S, 2), dtype=np.uint64)
        member = np.zeros((E, len(sh), 2), dtype=np.uint64)
        q = lambda a: p(a) if a.size else None
        self._check(self.lib.pantax_hip_strain_rarefy(self.ctx, self.db, self.reads, C.byref(cs), q(x), q(obj), q(rows), q(status), q(reads), q(member)))
        return x, obj, rows, status, reads, member

    def rarefy_node_bases(self, seed, replicate, level):
        """pantax_hip_rarefy_node_bases: bases_per_node of the reads of ONE level (0: every read) of a replicate, over every species -> uint64 [V]"""
        out = np.zeros(max(self.V, 1), dtype=np.uint64)
        self._check(self.lib.pantax_hip_rarefy_node_bases(self.ctx, self.db, self.reads, int(seed), int(replicate), int(level), p(out)))
        return out[:self.V]

    def strain_addin(self, sel_off, sel_hap, cand_off, cand_hap):
        """Add-one test of the strain fit (pantax_hip_strain_addin) on the coverage result get_node_abundances left on the device.  sel_off / sel_hap and
        cand_off / cand_hap as for strain_near_miss.  Species s of K_s reported and J_s candidate haplotypes has W_s = K_s + J_s columns (the reported ones
        first) and J_s + 1 entries: 0 the refit with every candidate pinned to zero, c + 1 the fit with candidate c free; entry (s, e) is
        q = cand_off[s] + s + e -> (x: list of S float64 [J_s + 1, W_s] blocks (views of one array, x[0].base), obj float64 [Q], status int32 [Q],
        rows uint64 [S], count uint64 [Q, 4] = n_member, n_novel, n_better, n_worse) with Q = cand_off[-1] + S."""
        so, sh = as_c(sel_off, np.uint64), as_c(sel_hap, np.uint32)
        co, ch = as_c(cand_off, np.uint64), as_c(cand_hap, np.uint32)
        if len(so) != self.S + 1 or len(sh) != int(so[-1]) or len(co) != self.S + 1 or len(ch) != int(co[-1]):
            raise ValueError("strain_addin: sel_off / cand_off need S + 1 entries, sel_hap sel_off[-1] and cand_hap cand_off[-1]")
        K, J = np.diff(so.astype(np.int64)), np.diff(co.astype(np.int64))
        x_off = np.concatenate([[0], np.cumsum((J + 1) * (K + J))]).astype(np.int64)
        Q = len(ch) + self.S
        cs = _ffi.NearMissSet(self.S, so.ctypes.data, sh.ctypes.data if len(sh) else None, co.ctypes.data, ch.ctypes.data if len(ch) else None)
        flat = np.zeros(max(int(x_off[-1]), 1), dtype=np.float64)
        obj = np.zeros(Q, dtype=np.float64)
        status = np.zeros(Q, dtype=np.int32)
        rows = np.zeros(self.S, dtype=np.uint64)
        count = np.zeros((Q, 4), dtype=np.uint64)
        self._check(self.lib.pantax_hip_strain_addin(self.ctx, self.db, C.byref(cs), p(flat), p(obj) if self.S else None, p(status) if self.S else None,
                                                     p(rows) if self.S else None, p(count) if self.S else None))
        flat = flat[:int(x_off[-1])]
        x = [flat[int(x_off[s]):int(x_off[s + 1])].reshape(int(J[s]) + 1, int(K[s] + J[s])) for s in range(self.S)]
        return x, obj, status, rows, count

    def hap_pairs(self, sel_off, sel_hap, species=True):
        """Pairwise strain distinguishability (pantax_hip_db_hap_pairs) of the resident db: no reads, no coverage pass.  sel_off [S+1], sel_hap as for
        strain_evidence (at most 256 haplotypes a species) -> (pair_off uint64 [S+1], pair uint64 [pair_off[-1], 2]: the K_s x K_s block of species s
        from pair_off[s], row-major, {n_nodes, len} of the nodes both haplotypes walk, species uint64 [S, 3, 2]: total / none / core).  species=False:
        the species sums are not fetched (species_out = NULL) and None is returned in their place."""
        so = as_c(sel_off, np.uint64)
        sh = as_c(sel_hap, np.uint32)
        if len(so) != self.S + 1 or len(sh) != int(so[-1]):
            raise ValueError("hap_pairs: sel_off needs S + 1 entries and sel_hap sel_off[-1]")
        cs = _ffi.EvidenceSet(self.S, so.ctypes.data, sh.ctypes.data if len(sh) else None)
        pair_off = np.zeros(self.S + 1, dtype=np.uint64)
        rc = self.lib.pantax_hip_db_hap_pairs(self.ctx, self.db, C.byref(cs), p(pair_off), 0, None, None)   # sizes the array
        if rc != _ffi.E_LIMIT:
            self._check(rc)
        n = int(pair_off[-1])
        pair = np.zeros((n, 2), dtype=np.uint64)
        sp = np.zeros((self.S, 3, 2), dtype=np.uint64) if species else None
        self._check(self.lib.pantax_hip_db_hap_pairs(self.ctx, self.db, C.byref(cs), p(pair_off), n, p(pair) if n else None, p(sp) if species and self.S else None))
        return pair_off, pair, sp

    def pair_evidence(self, sel_off, sel_hap, species=True):
        """Pairwise strain evidence (pantax_hip_strain_pair_evidence) of the coverage result get_node_abundances left on the device.  sel_off [S+1],
        sel_hap as for strain_evidence (at most 256 haplotypes a species) -> (pair_off uint64 [S+1], pair uint64 [pair_off[-1], 4]: the K_s x K_s block
        of species s from pair_off[s], row-major, {n_nodes, len, covered, bases} of the nodes both haplotypes walk, species uint64 [S, 3, 4]: total /
        orphan / core).  species=False: the species sums are not fetched (species_out = NULL) and None is returned in their place."""
        so = as_c(sel_off, np.uint64)
        sh = as_c(sel_hap, np.uint32)
        if len(so) != self.S + 1 or len(sh) != int(so[-1]):
            raise ValueError("pair_evidence: sel_off needs S + 1 entries and sel_hap sel_off[-1]")
        cs = _ffi.EvidenceSet(self.S, so.ctypes.data, sh.ctypes.data if len(sh) else None)
        pair_off = np.zeros(self.S + 1, dtype=np.uint64)
        rc = self.lib.pantax_hip_strain_pair_evidence(self.ctx, self.db, C.byref(cs), p(pair_off), 0, None, None)   # sizes the array
        if rc != _ffi.E_LIMIT:
            self._check(rc)
        n = int(pair_off[-1])
        pair = np.zeros((n, 4), dtype=np.uint64)
        sp = np.zeros((self.S, 3, 4), dtype=np.uint64) if species else None
        self._check(self.lib.pantax_hip_strain_pair_evidence(self.ctx, self.db, C.byref(cs), p(pair_off), n, p(pair) if n else None, p(sp) if species and self.S else None))
        return pair_off, pair, sp

    def trio_nodes_info(self, fetch=True):
        n = C.c_uint64(0)
        self._check(self.lib.pantax_hip_trio_index(self.ctx, self.db, C.byref(n)))
        self.U = n.value
        if not fetch:
            return self.U
        U = self.U
        abc = np.zeros(max(U, 1) * 3, dtype=np.uint32)
        hap = np.zeros(max(U, 1), dtype=np.uint32)
        ln = np.zeros(max(U, 1), dtype=np.int64)
        hto = np.zeros(self.H + 1, dtype=np.uint64)
        self._check(self.lib.pantax_hip_trio_get(self.ctx, self.db, p(abc), p(hap), p(ln), p(hto)))
        return abc[: 3 * U].reshape(-1, 3), hap[:U], ln[:U], hto

    def get_node_abundances(self, species_active=None, fetch=True, with_trio=True):
        """-> bases_per_node [V] int64, node_base_cov [V] uint64, trio_bases [U] int64, n_abort"""
        act = None if species_active is None else as_c(species_active, np.uint8)
        n_abort = C.c_uint64(0)
        if not fetch:   # results stay resident for strain_profiling; no host round trip
            self._check(self.lib.pantax_hip_node_coverage(self.ctx, self.db, self.reads, p(act), None, None, None, None))
            return None
        bases = np.zeros(self.V, dtype=np.int64)
        cov = np.zeros(self.V, dtype=np.uint64)
        tb = None
        if with_trio and self.U is not None:
            tb = np.zeros(max(self.U, 1), dtype=np.int64)
        self._check(self.lib.pantax_hip_node_coverage(self.ctx, self.db, self.reads, p(act), p(bases), p(cov), p(tb),
                                                      C.byref(n_abort)))
        return bases, cov, (tb[: self.U] if tb is not None else None), n_abort.value

    def strain_profiling(self, species_coverage, species_active=None, fr=0.3, fc=0.46, sr=0.85, min_depth=0,
                         shift=False, sample_nodes=0, solver_semantics=0):
        """solver_semantics: 0 = Gurobi's handling of the second solve (profile.rs:1500-1508), 1 = highs_opt's (profile.rs:2865-2879)"""
        cfg = _ffi.StrainConfig(fr, fc, sr, min_depth, int(shift), sample_nodes, int(solver_semantics))
        act = None if species_active is None else as_c(species_active, np.uint8)
        cov = as_c(species_coverage, np.float64)
        met = (_ffi.HapMetrics * max(self.H, 1))()
        info = (_ffi.SolveInfo * self.S)()
        self._check(self.lib.pantax_hip_strain_profile(self.ctx, self.db, C.byref(cfg), p(act), p(cov), met, info))
        return met, info

    def profile_step(self, avg_len, fr=0.3, fc=0.46, sr=0.85, sd=0.2, min_cov=0, min_depth=0, shift=False, filtered=True,
                     rebuild_trio=True, sample_nodes=0, solver_semantics=0):
        """One resident pass of the hot path in a single call (pantax_hip_profile_step): the host waits once.
        -> keep [S] uint8, predicted_coverage [S], metrics [H], info [S], pass [H] uint8, sum_all [S], sum_pass [S]"""
        if self._step_buf is None or self._step_buf[0] != (self.S, self.H):
            self._step_buf = ((self.S, self.H), np.zeros(self.S, dtype=np.uint8), np.zeros(self.S),
                              (_ffi.HapMetrics * max(self.H, 1))(), (_ffi.SolveInfo * self.S)(),
                              np.zeros(max(self.H, 1), dtype=np.uint8), np.zeros(self.S), np.zeros(self.S))
            self._step_ptr = [p(a) if isinstance(a, np.ndarray) else a for a in self._step_buf[1:]]
        _, keep, absolute, met, info, passed, s_all, s_pass = self._step_buf
        avg = as_c(avg_len, np.float64)
        cfg = _ffi.StepConfig(fr, fc, sr, sd, min_cov, min_depth, int(shift), int(filtered), int(sample_nodes), int(rebuild_trio), int(solver_semantics))
        self._check(self.lib.pantax_hip_profile_step(self.ctx, self.db, self.reads, p(avg), C.byref(cfg), *self._step_ptr))
        if rebuild_trio:
            self.U = None
        return keep, absolute, met, info, passed[: self.H], s_all, s_pass

    def trio_index_prefetch(self):
        """pantax_hip_trio_index_prefetch: the unique-trio index of the COMING step is started now (side stream), e.g. before that
        run's reads are loaded; the next step with rebuild_trio uses it instead of building again."""
        self._check(self.lib.pantax_hip_trio_index_prefetch(self.ctx, self.db))
        self.U = None

    def profile_step_enqueue(self, avg_len, fr=0.3, fc=0.46, sr=0.85, sd=0.2, min_cov=0, min_depth=0, shift=False, filtered=True,
                             rebuild_trio=True, sample_nodes=0, solver_semantics=0):
        """First half of profile_step (pantax_hip_profile_step_enqueue): the whole step goes onto the device, nothing is waited
        for.  Up to two steps may be in flight; the device runs their main-stream work one step after the other (the unique-trio
        rebuild of the next step may start behind the previous step's first filter, its last reader)."""
        avg = as_c(avg_len, np.float64)
        cfg = _ffi.StepConfig(fr, fc, sr, sd, min_cov, min_depth, int(shift), int(filtered), int(sample_nodes), int(rebuild_trio), int(solver_semantics))
        self._check(self.lib.pantax_hip_profile_step_enqueue(self.ctx, self.db, self.reads, p(avg), C.byref(cfg)))
        self._inflight += 1
        if rebuild_trio:
            self.U = None

    def profile_step_collect(self):
        """Second half: the oldest enqueued step's host wait + results (same tuple as profile_step).  The arrays are reused by
        the collect after next: copy what must live longer."""
        if self._collect_buf is None or self._collect_buf[0] != (self.S, self.H):
            mk = lambda: (np.zeros(self.S, dtype=np.uint8), np.zeros(self.S), (_ffi.HapMetrics * max(self.H, 1))(), (_ffi.SolveInfo * self.S)(),
                          np.zeros(max(self.H, 1), dtype=np.uint8), np.zeros(self.S), np.zeros(self.S))
            sets = [mk(), mk()]
            self._collect_buf = ((self.S, self.H), sets, [[p(a) if isinstance(a, np.ndarray) else a for a in st] for st in sets], 0)
        key, sets, ptrs, turn = self._collect_buf
        self._collect_buf = (key, sets, ptrs, turn ^ 1)
        keep, absolute, met, info, passed, s_all, s_pass = sets[turn]
        self._inflight = max(self._inflight - 1, 0)           # the library frees the slot also when the step reports a failure
        self._check(self.lib.pantax_hip_profile_step_collect(self.ctx, self.db, *ptrs[turn]))
        return keep, absolute, met, info, passed[: self.H], s_all, s_pass

    def drain_steps(self):
        """collect (and drop) whatever enqueued steps are still in flight, e.g. after an exception between enqueue and collect"""
        while self._inflight:
            try:
                self.profile_step_collect()
            except PantaxHipError:
                pass

    def pao_solve(self, node_len, node_abundance, node_base_cov, path_off, path_nodes, cand, fixed_zero=None):
        node_len = as_c(node_len, np.int64)
        ab = as_c(node_abundance, np.float64)
        cov = as_c(node_base_cov, np.uint64)
        path_off = as_c(path_off, np.uint64)
        path_nodes = as_c(path_nodes, np.uint32)
        cand = as_c(cand, np.uint32)
        fz = None if fixed_zero is None else as_c(fixed_zero, np.uint8)
        x = np.zeros(len(cand))
        ratio = np.zeros(len(cand), dtype=np.float32)
        obj = C.c_double(0)
        st = C.c_int32(0)
        self._check(self.lib.pantax_hip_pao_solve(self.ctx, C.c_uint32(len(node_len)), p(node_len), p(ab), p(cov),
                                                  C.c_uint32(len(path_off) - 1), p(path_off), p(path_nodes),
                                                  C.c_uint32(len(cand)), p(cand), p(fz), p(x), p(ratio),
                                                  C.byref(obj), C.byref(st)))
        return x, ratio, obj.value, st.value

    def pao_solve_batch(self, species, fixed_zero=None):
        """The solver seam for many species in ONE call (pantax_hip_pao_solve_batch).  species: list of
        (node_len, node_abundance, node_base_cov or None, path_off, path_nodes, cand) per species; fixed_zero: list of
        per-species uint8 arrays or None.  -> list of (x, ratio, obj, status, iters) per species."""
        S = len(species)
        node_off = np.zeros(S + 1, dtype=np.uint64); hap_off = np.zeros(S + 1, dtype=np.uint64); cand_off = np.zeros(S + 1, dtype=np.uint64)
        node_off[1:] = np.cumsum([len(sp[0]) for sp in species])
        hap_off[1:] = np.cumsum([len(sp[3]) - 1 for sp in species])
        cand_off[1:] = np.cumsum([len(sp[5]) for sp in species])
        node_len = as_c(np.concatenate([sp[0] for sp in species]), np.int64)
        ab = as_c(np.concatenate([sp[1] for sp in species]), np.float64)
        cov = as_c(np.concatenate([np.zeros(len(sp[0]), dtype=np.uint64) if sp[2] is None else sp[2] for sp in species]), np.uint64)
        offs, base = [np.zeros(1, dtype=np.uint64)], 0
        for sp in species:
            po = np.asarray(sp[3], dtype=np.uint64)
            offs.append(po[1:] + np.uint64(base)); base += int(po[-1])
        path_off = as_c(np.concatenate(offs), np.uint64)
        path_nodes = as_c(np.concatenate([sp[4] for sp in species]), np.uint32)
        cand = as_c(np.concatenate([np.asarray(sp[5], dtype=np.uint32) for sp in species]), np.uint32)
        fz = None
        if fixed_zero is not None:
            fz = as_c(np.concatenate([np.zeros(len(sp[5]), dtype=np.uint8) if f is None else f for sp, f in zip(species, fixed_zero)]), np.uint8)
        Cn = len(cand)
        x = np.zeros(max(Cn, 1)); ratio = np.zeros(max(Cn, 1), dtype=np.float32)
        obj = np.zeros(S); st = np.zeros(S, dtype=np.int32); it = np.zeros(S, dtype=np.int32)
        bi = _ffi.SpeciesBatch(S, p(node_off), p(node_len), p(ab), p(cov), p(hap_off), p(path_off), p(path_nodes), p(cand_off), p(cand), p(fz))
        bo = _ffi.SolutionBatch(p(x), p(ratio), p(obj), p(st), p(it))
        self._check(self.lib.pantax_hip_pao_solve_batch(self.ctx, C.byref(bi), C.byref(bo)))
        co = cand_off.astype(np.int64)
        return [(x[co[s]:co[s + 1]].copy(), ratio[co[s]:co[s + 1]].copy(), float(obj[s]), int(st[s]), int(it[s])) for s in range(S)]

    # ------------------------------------------------------------------ pipeline seam
    def profile(self, db, wd, gaf, species=True, strain=True, output_dir=None, fr=0.3, fc=0.46, sr=0.85, sd=0.2,
                min_species_abundance=1e-4, min_cov=0, min_depth=0, shift=False, filtered=True, full=True, force=False,
                mode=2, sample_nodes=0, designated_species=None, zip="serialize", out_binning_file=None,
                reads_binning_file=None, range_file=None, species_len_file=None, image_cache=0, rank=0, world_size=1,
                allreduce=None, alltoallv=None, sample_test=False, solver_semantics=0, minimization_min_cov=0.0, read_strain_file=None,
                strain_coverage_file=None, strain_coverage_window=0, strain_evidence_file=None, strain_read_support_file=None,
                strain_depth_file=None, strain_near_miss_file=None, strain_near_miss_top=0, strain_pair_evidence_file=None, strain_fit_file=None,
                strain_bootstrap_file=None, strain_bootstrap_replicates=0, strain_bootstrap_seed=42, strain_dropout_file=None,
                strain_addin_file=None, strain_addin_top=0, strain_em_file=None, strain_em_classes=0, strain_em_iterations=0,
                strain_segments_file=None, strain_segments_min=0, strain_segments_bridge=None, strain_segments_peak=0,
                strain_mosaic_file=None, strain_mosaic_top=0, strain_rescue_file=None, strain_rescue_top=0,
                strain_links_file=None, strain_links_top=0,
                strain_rarefy_file=None, strain_rarefy_levels=0, strain_rarefy_replicates=0, strain_rarefy_seed=42, strain_fragments_file=None,
                strain_growth_file=None, strain_growth_window=0, strain_growth_min_own=0, strain_growth_trim=0):
        """profile::profile(ProfilingConfig) (profile.rs:3325): files in, files out.  allreduce(float64 array) sums in place over
        the ranks; alltoallv(send uint8 array, send_off [W+1], recv uint8 array, recv_off [W+1]) moves bytes between the ranks
        (host buffers) and switches on the sharded ingest.  read_strain_file: path of the per-read strain report
        (--read-strains; one rank only).  strain_coverage_file: path of the per-strain windowed coverage track (--strain-coverage; one rank
        only), strain_coverage_window its window in bases (0: 10000).  strain_evidence_file: path of the per-strain node evidence report
        (--strain-evidence; one rank only).  strain_read_support_file: path of the per-strain read support report (--strain-read-support; one rank only).
        strain_depth_file: path of the per-strain depth distribution report (--strain-depth; one rank only).  strain_near_miss_file: path of the
        unreported-strain near-miss report (--strain-near-miss; one rank only), strain_near_miss_top the candidates it prints per species (0: 5).
        strain_pair_evidence_file: path of the pairwise strain evidence report (--strain-pair-evidence; one rank only).  strain_fit_file: path of the
        model fit report (--strain-fit; one rank only); given, the call goes through pantax_hip_profile_with_ext.  strain_bootstrap_file: path of the
        bootstrap report (--strain-bootstrap; one rank only), strain_bootstrap_replicates the resamples (0: 100), strain_bootstrap_seed their seed.  strain_dropout_file: path of
        the leave-one-out report (--strain-dropout; one rank only).  strain_addin_file: path of the add-one report (--strain-addin; one rank only),
        strain_addin_top the candidates it tests per species (0: 5).  strain_em_file: path of the read class report (--strain-em; one rank only),
        strain_em_classes the classes it prints per species (0: 10), strain_em_iterations the iterations of its estimate at most (0: 1000).
        strain_segments_file: path of the segment report (--strain-segments; one rank only), strain_segments_min the bases a chain spans at least
        (0: 1000), strain_segments_bridge the bases between two segments of a chain at most (None: 100; 0 is a bridge of 0 -- the struct holds
        bridge + 1), strain_segments_peak the integer factor F of peak_depth = max(2, ceil(F x predicted_coverage)) (0: 10; "off": no peak class).
        strain_mosaic_file: path of the mosaic read report (--strain-mosaic; one rank only), strain_mosaic_top the junctions it prints per species
        (0: 10; "off": none, and none are collected).
        strain_rescue_file: path of the read rescue report (--strain-rescue; one rank only), strain_rescue_top the candidates it prints per species (0: 5).
        strain_links_file: path of the link support report (--strain-links; one rank only), strain_links_top the breaks it prints per strain (0: 10).
        strain_rarefy_file: path of the rarefaction report (--strain-rarefy; one rank only), strain_rarefy_levels the thinned levels 1/2 .. 2^-N (0: 5; at
        most 16), strain_rarefy_replicates the replicates per level (0: 5), strain_rarefy_seed the seed of the thinning rule.
        strain_fragments_file: path of the fragment support report (--strain-fragments; one rank only).
        strain_growth_file: path of the replication index report (--strain-growth; one rank only), strain_growth_window its window in bases (0: 5000),
        strain_growth_min_own the own bases a window needs in thousandths of the window (0: 500), strain_growth_trim the windows trimmed from each end of
        the sorted range in thousandths (0: 100; below 500)."""
        enc = lambda x: None if x is None else str(x).encode()
        cfg = _ffi.ProfilingConfig(
            db=enc(db), wd=enc(wd), output_dir=enc(output_dir or wd), genomes_metadata=None, range_file=enc(range_file),
            input_aln_file=enc(gaf), species_len_file=enc(species_len_file), out_binning_file=enc(out_binning_file),
            reads_binning_file=enc(reads_binning_file), min_species_abundance=min_species_abundance,
            unique_trio_nodes_fraction=fr, unique_trio_nodes_mean_count_f=fc, single_cov_ratio=sr, single_cov_diff=sd,
            min_cov=min_cov, min_depth=min_depth, species=int(species), strain=int(strain), shift=int(shift),
            filtered=int(filtered), full=int(full), force=int(force), mode=mode, sample_nodes=sample_nodes,
            designated_species=enc(designated_species), zip=enc(zip), rank=int(rank), world_size=int(world_size),
            image_cache=int(image_cache), sample_test=int(sample_test), solver_semantics=int(solver_semantics),
            minimization_min_cov=float(minimization_min_cov), read_strain_file=enc(read_strain_file),
            strain_coverage_file=enc(strain_coverage_file), strain_coverage_window=int(strain_coverage_window),
            strain_evidence_file=enc(strain_evidence_file), strain_read_support_file=enc(strain_read_support_file),
            strain_depth_file=enc(strain_depth_file), strain_near_miss_file=enc(strain_near_miss_file),
            strain_near_miss_top=int(strain_near_miss_top), strain_pair_evidence_file=enc(strain_pair_evidence_file))
        cb = None
        if allreduce is not None:   # allreduce(np.ndarray float64) sums it in place over the ranks
            def _cb(_user, buf, n):
                try:
                    allreduce(np.ctypeslib.as_array(buf, shape=(int(n),)))
                    return 0
                except Exception:   # noqa: BLE001 -- reported through the return code
                    return 1
            cb = _ffi.ALLREDUCE_FN(_cb)
            cfg.allreduce_sum = C.cast(cb, C.c_void_p)
        cb2 = None
        if alltoallv is not None:
            W = int(world_size)

            def _cb2(_user, send, send_off, recv, recv_off):
                try:
                    so = np.ctypeslib.as_array(send_off, shape=(W + 1,)).astype(np.int64)
                    ro = np.ctypeslib.as_array(recv_off, shape=(W + 1,)).astype(np.int64)
                    sb = (np.ctypeslib.as_array(C.cast(send, C.POINTER(C.c_uint8)), shape=(int(so[-1]),)) if so[-1] else np.zeros(0, dtype=np.uint8))
                    rb = (np.ctypeslib.as_array(C.cast(recv, C.POINTER(C.c_uint8)), shape=(int(ro[-1]),)) if ro[-1] else np.zeros(0, dtype=np.uint8))
                    alltoallv(sb, so, rb, ro)
                    return 0
                except Exception:   # noqa: BLE001 -- reported through the return code
                    return 1
            cb2 = _ffi.ALLTOALLV_FN(_cb2)
            cfg.alltoallv = C.cast(cb2, C.c_void_p)
            cfg.comm_device_buffers = 0
        if strain_fit_file is None and strain_bootstrap_file is None and strain_dropout_file is None and strain_addin_file is None and strain_em_file is None and strain_segments_file is None and strain_mosaic_file is None and strain_rescue_file is None and strain_links_file is None and strain_rarefy_file is None and strain_fragments_file is None and strain_growth_file is None:
            self._check(self.lib.pantax_hip_profile(self.ctx, C.byref(cfg)))
        else:   # the outputs behind the config's last field travel in the sized extension
            ext = _ffi.ProfileExt(struct_size=C.sizeof(_ffi.ProfileExt), strain_fit_file=enc(strain_fit_file), strain_bootstrap_file=enc(strain_bootstrap_file),
                                  strain_bootstrap_replicates=int(strain_bootstrap_replicates), strain_bootstrap_seed=int(strain_bootstrap_seed),
                                  strain_dropout_file=enc(strain_dropout_file), strain_addin_file=enc(strain_addin_file), strain_addin_top=int(strain_addin_top),
                                  strain_em_file=enc(strain_em_file), strain_em_classes=int(strain_em_classes), strain_em_iterations=int(strain_em_iterations),
                                  strain_segments_file=enc(strain_segments_file), strain_segments_min=int(strain_segments_min),
                                  strain_segments_bridge=0 if strain_segments_bridge is None else int(strain_segments_bridge) + 1,
                                  strain_segments_peak=_ffi.SEGMENTS_PEAK_OFF if strain_segments_peak == "off" else int(strain_segments_peak),
                                  strain_mosaic_file=enc(strain_mosaic_file),
                                  strain_mosaic_top=_ffi.MOSAIC_TOP_OFF if strain_mosaic_top == "off" else int(strain_mosaic_top),
                                  strain_rescue_file=enc(strain_rescue_file), strain_rescue_top=int(strain_rescue_top),
                                  strain_links_file=enc(strain_links_file), strain_links_top=int(strain_links_top),
                                  strain_rarefy_file=enc(strain_rarefy_file), strain_rarefy_levels=int(strain_rarefy_levels),
                                  strain_rarefy_replicates=int(strain_rarefy_replicates), strain_rarefy_seed=int(strain_rarefy_seed),
                                  strain_fragments_file=enc(strain_fragments_file), strain_growth_file=enc(strain_growth_file),
                                  strain_growth_window=int(strain_growth_window), strain_growth_min_own_permille=int(strain_growth_min_own),
                                  strain_growth_trim_permille=int(strain_growth_trim))
            self._check(self.lib.pantax_hip_profile_with_ext(self.ctx, C.byref(cfg), C.byref(ext)))

    def db_pairs(self, db, out_file, species=None, max_distance=None, zip="serialize", range_file=None):
        """pantax_hip_db_pairs (the --db-pairs mode): the pairwise distinguishability table of a db directory -> out_file.  species: taxids (a list or a
        comma-separated string; None = every species with more than one haplotype); max_distance: only pairs at most that many bases apart (None:
        all); zip: "serialize" / "lz" / "zstd", None = GFA text."""
        enc = lambda x: None if x is None else str(x).encode()
        if species is not None and not isinstance(species, str):
            species = ",".join(str(x) for x in species)
        cfg = _ffi.DbPairsConfig(db=enc(db), out_file=enc(out_file), range_file=enc(range_file), species=enc(species), zip=enc(zip),
                                 max_distance=-1 if max_distance is None else int(max_distance))
        self._check(self.lib.pantax_hip_db_pairs(self.ctx, C.byref(cfg)))

    def save_images(self, paths, hap_names):
        """one device-ready image per species of the resident db: the graph alone (node lengths, walk offsets, packed walks,
        haplotype names; format 4, db_image.cpp).  The arrays are downloaded from the device, so the files are the read-back of whatever route
        uploaded the db."""
        ps = (C.c_char_p * self.S)(*[x.encode() for x in paths])
        hn = (C.c_char_p * max(self.H, 1))(*[x.encode() for x in hap_names])
        self._check(self.lib.pantax_hip_db_save_images(self.ctx, self.db, ps, hn))

    def load_images(self, paths, range_start, range_end, species):
        """Resident db from images; `species` (the same graphs as objects) only supplies the host-side shapes the
        wrapper keeps (node_off, hap_off) -- nothing of it is uploaded."""
        if self.db:
            self.lib.pantax_hip_db_free(self.ctx, self.db)
            self.db = None
            self._inflight = 0
        S = len(paths)
        self.S = S
        self.range_start = as_c(range_start, np.int64)
        self.range_end = as_c(range_end, np.int64)
        self.node_off = np.zeros(S + 1, dtype=np.uint64)
        self.node_off[1:] = np.cumsum([len(g.node_len) for g in species])
        self.hap_off = np.zeros(S + 1, dtype=np.uint64)
        self.hap_off[1:] = np.cumsum([len(g.path_off) - 1 for g in species])
        self.V, self.H = int(self.node_off[-1]), int(self.hap_off[-1])
        ps = (C.c_char_p * S)(*[x.encode() for x in paths])
        db = C.c_void_p()
        self._check(self.lib.pantax_hip_db_load_images(self.ctx, C.c_uint32(S), ps, p(self.range_start), p(self.range_end), C.byref(db)))
        self.db = db
        self.U = None

    def gaf_filter(self, gaf_path, out_path=None):
        """filter_max_alignment_mt (gaf_filter.rs:44-97) on the device -> (lines, records, lines written)."""
        nl, nr, nw = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.pantax_hip_gaf_filter(self.ctx, gaf_path.encode(), out_path.encode() if out_path else None,
                                                   C.byref(nl), C.byref(nr), C.byref(nw)))
        return nl.value, nr.value, nw.value

    @staticmethod
    def sample_ranks(n_valid, sample_nodes, seed=42):
        """a11: bool [n_valid], True where sample_sorted (profile.rs:1287-1295) keeps the row of that rank.  Host only."""
        bits = np.zeros((n_valid + 31) // 32, dtype=np.uint32)
        rc = _ffi.load().pantax_hip_sample_ranks(C.c_uint64(n_valid), C.c_uint64(sample_nodes), C.c_uint64(seed), p(bits))
        if rc != 0:
            raise ValueError("sample_ranks(%d, %d)" % (n_valid, sample_nodes))
        return np.unpackbits(bits.view(np.uint8), bitorder="little")[:n_valid].astype(bool)

    @staticmethod
    def chacha_block(key8, counter, rounds):
        key = np.ascontiguousarray(key8, dtype=np.uint32)
        out = np.zeros(16, dtype=np.uint32)
        if _ffi.load().pantax_hip_chacha_block(p(key), C.c_uint64(counter), int(rounds), p(out)) != 0:
            raise ValueError("chacha_block")
        return out

    # ------------------------------------------------------------------ timing
    def sort_rows(self, k0, k1, k2, algo=0):
        """Sort the rows (k0[i], k1[i], k2[i]) ascending as tuples on the device (0 auto, 1 radix, 2 sample sort)."""
        k = [np.ascontiguousarray(x, dtype=np.uint64).copy() for x in (k0, k1, k2)]
        self._check(self.lib.pantax_hip_sort_rows(self.ctx, C.c_uint64(len(k[0])), p(k[0]), p(k[1]), p(k[2]), int(algo)))
        return k

    def scan(self, x, in_place=False):
        """pantax_hip_scan: the chained exclusive scan of a uint8 or uint32 array in 32-bit arithmetic -> (out uint32 [n], total, items per workgroup of the
        launch).  in_place (uint32 only): the device scan reads and writes one buffer."""
        x = np.ascontiguousarray(x)
        if x.dtype not in (np.uint8, np.uint32):
            raise TypeError("scan takes uint8 or uint32 items, not %s" % x.dtype)
        out = np.empty(len(x), dtype=np.uint32)
        total, tile = C.c_uint32(0), C.c_uint32(0)
        self._check(self.lib.pantax_hip_scan(self.ctx, len(x), p(x), x.dtype.itemsize, int(bool(in_place)), p(out), C.byref(total), C.byref(tile)))
        return out, total.value, tile.value

    def radix_sort(self, keys, passes, payload=None, n_actual=None):
        """pantax_hip_radix_sort: the records (keys[0][i], .. keys[nw - 1][i][, payload[i]]), nw = 1 .. 3, through the stable LSD radix sort over the digits
        passes = [(word, shift), ..], least significant first.  n_actual (default: all) is the record count the device is given while len(keys[0]) fixes the
        launch geometry -> (key words, payload or None, True when the result ended on the second side)."""
        k = [np.ascontiguousarray(w, dtype=np.uint64).copy() for w in keys]
        n = len(k[0])
        v = None if payload is None else np.ascontiguousarray(payload, dtype=np.uint32).copy()
        pw = np.ascontiguousarray([w for w, _ in passes], dtype=np.int32)
        ps = np.ascontiguousarray([s for _, s in passes], dtype=np.int32)
        in_b = C.c_int(0)
        kp = [p(w) for w in k] + [None] * (3 - len(k))
        self._check(self.lib.pantax_hip_radix_sort(self.ctx, n, n if n_actual is None else int(n_actual), len(k), kp[0], kp[1], kp[2], p(v), p(pw), p(ps), len(passes),
                                                   C.byref(in_b)))
        return k, v, bool(in_b.value)

    def fill(self, buf_bytes, off, nbytes, byte, sentinel):
        """pantax_hip_fill: a device buffer of buf_bytes set to `sentinel`, then [off, off + nbytes) of it to `byte` by the library's fill -> the whole buffer"""
        out = np.empty(buf_bytes, dtype=np.uint8)
        self._check(self.lib.pantax_hip_fill(self.ctx, int(buf_bytes), int(sentinel), int(off), int(nbytes), int(byte), p(out)))
        return out

    def strain_node_stats(self):
        """pantax_hip_strain_node_stats: per-species (amax, nvalid, nzsum, nzcnt) of the strain step collected last, unrounded"""
        amax, nzsum = np.zeros(self.S), np.zeros(self.S)
        nvalid, nzcnt = np.zeros(self.S, dtype=np.uint32), np.zeros(self.S, dtype=np.uint32)
        self._check(self.lib.pantax_hip_strain_node_stats(self.ctx, self.db, p(amax), p(nvalid), p(nzsum), p(nzcnt)))
        return amax, nvalid, nzsum, nzcnt

    def strain_hap_stats(self):
        """pantax_hip_strain_hap_stats: per-haplotype (nnz, mean_filtered) of the strain step collected last, as the device left them"""
        nnz, meanf = np.zeros(max(self.H, 1), dtype=np.uint32), np.zeros(max(self.H, 1))
        self._check(self.lib.pantax_hip_strain_hap_stats(self.ctx, self.db, p(nnz), p(meanf)))
        return nnz[: self.H], meanf[: self.H]

    def strain_node_cov(self):
        """pantax_hip_strain_node_cov: (cov [V] uint32, ab [V] float64) of the strain step collected last, when it took the split node pass"""
        cov, ab = np.zeros(max(self.V, 1), dtype=np.uint32), np.zeros(max(self.V, 1))
        self._check(self.lib.pantax_hip_strain_node_cov(self.ctx, self.db, p(cov), p(ab)))
        return cov[: self.V], ab[: self.V]

    def timing_enable(self, on=True):
        self._check(self.lib.pantax_hip_timing_enable(self.ctx, int(on)))

    def timing_filter(self, name=None):
        self._check(self.lib.pantax_hip_timing_filter(self.ctx, name.encode() if name else None))

    def timing_reset(self):
        self._check(self.lib.pantax_hip_timing_reset(self.ctx))

    def timing_get(self):
        cap = 256    # (a resident step launches more than 64 differently named kernels once the index rebuild is in it: the table was cut short)
        names = (C.c_char_p * cap)()
        launches = (C.c_uint64 * cap)()
        ms = (C.c_double * cap)()
        n = self.lib.pantax_hip_timing_get(self.ctx, cap, names, launches, ms)
        if n < 0:
            self._check(n)
        return {names[i].decode(): (int(launches[i]), float(ms[i])) for i in range(min(n, cap))}


def depth_bin(d):
    """pantax_hip_depth_bin: the histogram bin (0 .. 95) of a node depth (any integer 0 <= d < 2^64).  Host only: no Engine is needed."""
    return int(_ffi.load().pantax_hip_depth_bin(int(d)))


def bootstrap_weight(seed, sp_key, replicate, v_local):
    """pantax_hip_bootstrap_weight: the weight (0 .. 16) of node v_local of the species with key sp_key in bootstrap replicate `replicate` (0: always 1).
    Host only: no Engine is needed."""
    return int(_ffi.load().pantax_hip_bootstrap_weight(int(seed), int(sp_key), int(replicate), int(v_local)))


def dropout_substitute(k, x_full, x_drop):
    """pantax_hip_dropout_substitute: who takes over when column k is dropped.  x_full / x_drop float64 [K]: the x of the plain refit and of the fit without
    column k -> (substitute column or -1, its gain, shift = the L1 distance of the two solutions over the other columns)."""
    xf, xd = as_c(x_full, np.float64), as_c(x_drop, np.float64)
    if xf.ndim != 1 or xf.shape != xd.shape:
        raise ValueError("dropout_substitute: x_full and x_drop are one-dimensional and of one length")
    out = np.zeros(3, dtype=np.float64)
    if _ffi.load().pantax_hip_dropout_substitute(len(xf), int(k), p(xf), p(xd), p(out)) != 0:
        raise ValueError("dropout_substitute: refused")
    return int(out[0]), float(out[1]), float(out[2])


def read_em(mask, b, length, max_iter=1000, tol=1e-6):
    """pantax_hip_read_em: the read-based estimate of one species on the host.  mask / b uint64 [J]: the classes in ascending mask and their spans;
    length uint64 [K]: the graph bases of the candidates in ascending haplotype index (bit k of a mask) -> (x float64 [K], n_iter, converged, delta)."""
    m = as_c(mask, np.uint64)
    bb = as_c(b, np.uint64)
    ln = as_c(length, np.uint64)
    if m.ndim != 1 or bb.shape != m.shape or ln.ndim != 1:
        raise ValueError("read_em: mask and b are one-dimensional and of one length, length is one-dimensional")
    x = np.zeros(len(ln), dtype=np.float64)
    n_iter, conv, delta = C.c_uint32(0), C.c_int32(0), C.c_double(0.0)
    if _ffi.load().pantax_hip_read_em(len(ln), len(m), p(m), p(bb), p(ln), int(max_iter), float(tol), p(x), C.byref(n_iter), C.byref(conv), C.byref(delta)) != 0:
        raise ValueError("read_em: refused")
    return x, int(n_iter.value), int(conv.value), float(delta.value)


GROWTH_STATUS = ("ok", "empty", "few_windows", "low_depth", "flat")   # PANTAX_HIP_GROWTH_*: the names the report prints


def growth_fit(len_own, bases_own, min_own, trim_permille=100, min_windows=_ffi.GROWTH_MIN_WINDOWS, min_depth=_ffi.GROWTH_MIN_DEPTH):
    """pantax_hip_growth_fit: the replication index over the own-node windows of ONE selection entry (Engine.strain_growth) -- keep the windows with
    len_own >= min_own, sort by depth as an exact rational, drop what lies outside [median / 8, median x 8], trim trim_permille thousandths from each
    end, fit log2 depth against rank.  -> dict(n_kept, n_zero, n_f, n_fit, own_len, median_depth, slope, intercept, r2, index, status), status one of
    GROWTH_STATUS.  ValueError where the library refuses (trim_permille >= 500, min_own = 0)."""
    ln = as_c(len_own, np.uint64)
    bs = as_c(bases_own, np.uint64)
    if len(ln) != len(bs):
        raise ValueError("growth_fit: the two arrays are of one length")
    if int(min_own) < 0 or int(trim_permille) < 0 or int(min_windows) < 0:
        raise ValueError("growth_fit: negative parameter")
    out = _ffi.GrowthFitResult()
    lib = _ffi.load()
    if lib.pantax_hip_growth_fit(len(ln), ln.ctypes.data if len(ln) else None, bs.ctypes.data if len(bs) else None, int(min_own), int(trim_permille),
                                 int(min_windows), float(min_depth), C.byref(out)) != 0:
        raise ValueError("growth_fit: refused")
    r = {k: getattr(out, k) for k in ("n_kept", "n_zero", "n_f", "n_fit", "own_len", "median_depth", "slope", "intercept", "r2", "index")}
    r["status"] = lib.pantax_hip_growth_status_name(out.status).decode()
    return r


def segment_chain(seg_class, seg_start, seg_len, seg_n_steps, seg_bases, bridge, min_span):
    """pantax_hip_segment_chain: chains of the segments of ONE haplotype (ascending start, disjoint).  Per class separately, consecutive segments at most
    `bridge` bases apart form a chain; those of span >= min_span are returned in ascending start -> (chain_class uint8 [M], first uint64 [M], last uint64
    [M]: its first and last member, q uint64 [M, 7]: start, end, span, in_class, n_segments, n_steps, bases)."""
    cl = as_c(seg_class, np.uint8)
    st = as_c(seg_start, np.uint64)
    ln = as_c(seg_len, np.uint64)
    ns = as_c(seg_n_steps, np.uint32)
    bs = as_c(seg_bases, np.uint64)
    n = len(cl)
    if not (len(st) == len(ln) == len(ns) == len(bs) == n):
        raise ValueError("segment_chain: the five arrays are of one length")
    c_cls = np.zeros(n, dtype=np.uint8)
    first, last = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    q = np.zeros((n, _ffi.SEGMENT_CHAIN_N), dtype=np.uint64)
    m = C.c_uint64(0)
    a = lambda x: p(x) if n else None
    if _ffi.load().pantax_hip_segment_chain(n, a(cl), a(st), a(ln), a(ns), a(bs), int(bridge), int(min_span), C.byref(m), a(c_cls), a(first), a(last), a(q)) != 0:
        raise ValueError("segment_chain: refused")
    m = int(m.value)
    return c_cls[:m].copy(), first[:m].copy(), last[:m].copy(), q[:m].copy()


def mosaic_walk(masks, w, hap, cap=None):
    """pantax_hip_mosaic_walk: the greedy cut of ONE walk.  masks uint64 [n]: bit p of masks[i] = the candidate at position p walks step i; w float64 [K],
    hap uint32 [K]: weight and haplotype index of position p, 1 <= K <= 64 -> (k, foreign_steps, seg_end uint64 [k]: segment j is the steps
    [seg_end[j-1], seg_end[j]), seg_pos uint32 [k]: the position it is assigned).  A foreign or empty walk has k = 0.  cap: the segments the arrays
    hold (None: n); a cap below k raises ValueError."""
    mk = as_c(masks, np.uint64)
    ww = as_c(w, np.float64)
    hh = as_c(hap, np.uint32)
    if len(ww) != len(hh):
        raise ValueError("mosaic_walk: w and hap are of one length")
    n = len(mk)
    cap = n if cap is None else int(cap)
    seg_end = np.zeros(cap, dtype=np.uint64)
    seg_pos = np.zeros(cap, dtype=np.uint32)
    k, fs = C.c_uint64(0), C.c_uint64(0)
    a = lambda x: p(x) if len(x) else None
    rc = _ffi.load().pantax_hip_mosaic_walk(n, a(mk), len(ww), a(ww), a(hh), a(seg_end), a(seg_pos), cap, C.byref(k), C.byref(fs))
    if rc != 0:
        raise ValueError("mosaic_walk: refused (%d)" % rc)
    k = int(k.value)
    return k, int(fs.value), seg_end[:k].copy(), seg_pos[:k].copy()


def mosaic_top(node_a, node_b, count, top):
    """pantax_hip_mosaic_top: the indices of the first `top` junctions in the order count descending, then node_a, then node_b ascending."""
    na = as_c(node_a, np.uint32)
    nb = as_c(node_b, np.uint32)
    ct = as_c(count, np.uint64)
    n = len(ct)
    if not (len(na) == len(nb) == n):
        raise ValueError("mosaic_top: the three arrays are of one length")
    idx = np.zeros(min(n, int(top)), dtype=np.uint64)
    m = C.c_uint64(0)
    a = lambda x: p(x) if len(x) else None
    if _ffi.load().pantax_hip_mosaic_top(n, a(na), a(nb), a(ct), int(top), a(idx), C.byref(m)) != 0:
        raise ValueError("mosaic_top: refused")
    return idx[:int(m.value)].copy()


def addin_donor(K, x_base, x_add):
    """pantax_hip_addin_donor: which reported strain gives coverage up when a candidate enters.  x_base / x_add float64 [W]: the x of entry 0 and of the
    candidate's entry, the first K columns the reported ones -> (donor column or -1, its loss, shift = the L1 distance of the two solutions over the
    reported columns)."""
    xb, xa = as_c(x_base, np.float64), as_c(x_add, np.float64)
    if xb.ndim != 1 or xb.shape != xa.shape:
        raise ValueError("addin_donor: x_base and x_add are one-dimensional and of one length")
    out = np.zeros(3, dtype=np.float64)
    if _ffi.load().pantax_hip_addin_donor(len(xb), int(K), p(xb), p(xa), p(out)) != 0:
        raise ValueError("addin_donor: refused")
    return int(out[0]), float(out[1]), float(out[2])


def bootstrap_summary(x, status=None):
    """pantax_hip_bootstrap_summary over the replicates b >= 1: x their values, status their LP statuses (None: all solved) -> float64 [10] = {n_solved, mean,
    sd, q025, q25, q50, q75, q975, zero_fraction, min}.  Host only."""
    xv = as_c(x, np.float64)
    st = None if status is None else as_c(status, np.int32)
    if xv.ndim != 1 or (st is not None and st.shape != xv.shape):
        raise ValueError("bootstrap_summary: x and status are one-dimensional and of one length")
    out = np.zeros(10, dtype=np.float64)
    if _ffi.load().pantax_hip_bootstrap_summary(len(xv), p(xv) if len(xv) else None, p(st) if st is not None and len(st) else None, p(out)) != 0:
        raise ValueError("bootstrap_summary: refused")
    return out


def depth_bin_range(b):
    """pantax_hip_depth_bin_range: (lo, hi) of bin b -- its depths are lo <= d < hi (bin 95: up to hi = 2^64 - 1).  ValueError for b > 95."""
    lo, hi = C.c_uint64(0), C.c_uint64(0)
    if _ffi.load().pantax_hip_depth_bin_range(int(b), C.byref(lo), C.byref(hi)) != 0:
        raise ValueError("depth_bin_range: bin %r" % (b,))
    return int(lo.value), int(hi.value)


def depth_quantile(hist, per_mille):
    """pantax_hip_depth_quantile: the bin of the length-weighted quantile of one histogram [96, 2] ({n_nodes, len} per bin), None when it holds no
    length.  ValueError for per_mille > 1000."""
    h = as_c(hist, np.uint64)
    if h.shape != (_ffi.DEPTH_BINS, 2):
        raise ValueError("depth_quantile: the histogram is [96, 2]")
    out = C.c_uint32(0)
    rc = _ffi.load().pantax_hip_depth_quantile(p(h), int(per_mille), C.byref(out))
    if rc == _ffi.DEPTH_NONE:
        return None
    if rc != 0:
        raise ValueError("depth_quantile: per_mille %r" % (per_mille,))
    return int(out.value)


def near_miss_rank(cand_hap, cand_out, top=0):
    """pantax_hip_near_miss_rank: the positions of one species' candidates (cand_hap [n], cand_out [n, 2, 4] of strain_near_miss) in the order of the
    report -- novel bases descending, then novel covered descending, then haplotype index ascending; candidates without novel bases are left out; the
    first `top` (0: all).  Host only: no Engine is needed."""
    ch = as_c(cand_hap, np.uint32)
    co = as_c(cand_out, np.uint64)
    if co.shape != (len(ch), 2, 4):
        raise ValueError("near_miss_rank: cand_out is [len(cand_hap), 2, 4]")
    out = np.zeros(max(len(ch), 1), dtype=np.uint32)
    n = C.c_uint32(0)
    one = np.zeros(8, dtype=np.uint64)   # (a zero-length array has no address to hand over)
    rc = _ffi.load().pantax_hip_near_miss_rank(len(ch), p(ch) if len(ch) else p(out), p(co) if len(ch) else p(one), int(top), p(out), C.byref(n))
    if rc != 0:
        raise ValueError("near_miss_rank: refused (%d)" % rc)
    return out[:n.value].copy()


def rescue_walk(sel_masks, cand_masks, K, J):
    """pantax_hip_rescue_walk: the read rescue classes of ONE walk.  sel_masks / cand_masks uint64 [n]: bit p = the member at position p of Sel / Cand walks
    step i (bits at and above K / J are ignored), K + J <= 64 -> (class: 0 compatible, 1 foreign_rescued, 2 foreign_patchwork, 3 foreign_novel,
    4 mosaic_rescued, 5 mosaic_unrescued; D(r) as a mask over Cand; steps uint64 [3] = foreign_steps, claimed_steps, novel_steps).  Host only."""
    sm = as_c(sel_masks, np.uint64)
    cm = as_c(cand_masks, np.uint64)
    if len(sm) != len(cm):
        raise ValueError("rescue_walk: sel_masks and cand_masks are of one length")
    cls, d = C.c_uint32(0), C.c_uint64(0)
    steps = np.zeros(3, dtype=np.uint64)
    a = lambda x: p(x) if len(x) else None
    rc = _ffi.load().pantax_hip_rescue_walk(len(sm), a(sm), a(cm), int(K), int(J), C.byref(cls), C.byref(d), p(steps))
    if rc != 0:
        raise ValueError("rescue_walk: refused (%d)" % rc)
    return int(cls.value), int(d.value), steps


def rescue_rank(cand_hap, cand_out, top=0):
    """pantax_hip_rescue_rank: the positions of one species' candidates (cand_hap [n], cand_out [n, 3, 3] of strain_read_rescue) in the order of the
    report -- rescued span descending, then rescued reads descending, then haplotype index ascending; candidates that rescue no read are left out; the
    first `top` (0: all).  Host only: no Engine is needed."""
    ch = as_c(cand_hap, np.uint32)
    co = as_c(cand_out, np.uint64)
    if co.shape != (len(ch), 3, 3):
        raise ValueError("rescue_rank: cand_out is [len(cand_hap), 3, 3]")
    out = np.zeros(max(len(ch), 1), dtype=np.uint32)
    n = C.c_uint32(0)
    one = np.zeros(9, dtype=np.uint64)   # (a zero-length array has no address to hand over)
    rc = _ffi.load().pantax_hip_rescue_rank(len(ch), p(ch) if len(ch) else p(out), p(co) if len(ch) else p(one), int(top), p(out), C.byref(n))
    if rc != 0:
        raise ValueError("rescue_rank: refused (%d)" % rc)
    return out[:n.value].copy()


def fragment_key(id_bytes):
    """pantax_hip_fragment_key: (key, tag) of a read id -- an id that ends in "/1" or "/2" behind a stem of at least one byte has the tag 1 or 2 and the
    id hash of the stem as its key; every other id has the tag 0 and its own id hash.  Host only: no Engine is needed."""
    b = bytes(id_bytes)
    key = C.c_uint64(0)
    tag = C.c_uint8(0)
    rc = _ffi.load().pantax_hip_fragment_key(b, len(b), C.byref(key), C.byref(tag))
    if rc != 0:
        raise ValueError("fragment_key: refused (%d)" % rc)
    return int(key.value), int(tag.value)


def rarefy_depth(seed, replicate, read):
    """pantax_hip_rarefy_depth: the depth (0 .. 63) of read `read` (its index in the uploaded columns) in replicate `replicate` of the rarefaction: the read
    belongs to level l iff depth >= l.  Host only: no Engine is needed."""
    return int(_ffi.load().pantax_hip_rarefy_depth(int(seed), int(replicate), int(read)))


def link_crossings(masks, known, K):
    """pantax_hip_link_crossings: the classes of the crossings of ONE walk.  masks uint64 [n]: bit p = the member at position p of the list walks step i
    (bits at and above K are ignored); known [n - 1]: non-zero where the crossing {step i, step i + 1} is a link of some member; K <= 64 ->
    uint64 [4] = known, skip, switch, foreign.  Host only."""
    m = as_c(masks, np.uint64)
    kn = as_c(known, np.uint8)
    if len(m) == 0 or len(kn) != len(m) - 1:
        raise ValueError("link_crossings: masks holds n >= 1 steps and known n - 1 crossings")
    out = np.zeros(4, dtype=np.uint64)
    rc = _ffi.load().pantax_hip_link_crossings(len(m), p(m), p(kn) if len(kn) else None, int(K), p(out))
    if rc != 0:
        raise ValueError("link_crossings: refused (%d)" % rc)
    return out


def link_top(flank, start, top=0):
    """pantax_hip_link_top: the indices of the first `top` (0: all) breaks in the order of the report -- flank descending, then start ascending.
    Host only: no Engine is needed."""
    fl = as_c(flank, np.uint64)
    st = as_c(start, np.uint64)
    if len(fl) != len(st):
        raise ValueError("link_top: flank and start are of one length")
    out = np.zeros(max(len(fl), 1), dtype=np.uint64)
    n = C.c_uint64(0)
    rc = _ffi.load().pantax_hip_link_top(len(fl), p(fl) if len(fl) else None, p(st) if len(fl) else None, int(top), p(out), C.byref(n))
    if rc != 0:
        raise ValueError("link_top: refused (%d)" % rc)
    return out[:n.value].copy()


def metrics_to_dicts(met, n=None):
    out = []
    for i, m in enumerate(met):
        if n is not None and i >= n:
            break
        d = {}
        for name, bit, attr in [("unique_trio_fraction", 1, "unique_trio_nodes_fraction"),
                                ("uniq_trio_cov_mean", 2, "frequencies_mean"), ("path_base_cov", 4, "path_cov_ratio"),
                                ("first_sol", 8, "first_sol"), ("strain_cov_diff", 16, "divergence"),
                                ("predicted_coverage", 32, "second_sol"), ("total_cov_diff", 128, "total_cov_diff")]:
            d[name] = getattr(m, attr) if m.has & bit else None
        d["is_rescue"] = bool(m.is_rescue) if m.has & 64 else None
        out.append(d)
    return out
