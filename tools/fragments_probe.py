#!/usr/bin/env python3
"""Measurement: the fragment support (pantax_hip_fragment_mates, pantax_hip_strain_fragments) on a bench workload, beside the per-strain read support
(pantax_hip_strain_read_support) on the same candidates in the same session.  Builds the set as bench.py does, runs one resident step and takes the
candidates from its rows (the a15 pass bits, weight = second_sol).  Every second read is renamed: two neighbours in the by-species order of the reads
share a 64-bit key (a hash of the pair's number) and carry the tags 1 and 2, so the reads form pairs as a paired-end sample would.  Times the kernels of
the three calls through timing_get and prints them with the classes' totals.
usage: fragments_probe.py [workload (cfg4)] [repeats (3)] [record.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import bench
from pantax_amd.engine import Engine

name = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 3
record = sys.argv[3] if len(sys.argv) > 3 else None
spec = bench.workload_spec(name)
t0 = time.perf_counter()
ns = bench.native_set(spec, threads=min(16, os.cpu_count() or 1))
rd = ns.reads()
species = ns.graphs()
avg = ns.avg_len()
print("%s: %d species, %d reads, %d steps, generated in %.1f s" % (name, len(species), rd.n_reads, len(rd.node_id), time.perf_counter() - t0), flush=True)
eng = Engine(0)
eng.upload_db(species)
eng.upload_packed(rd)
eng.rcls_profile(want_species=False)
eng.trio_nodes_info()
fr = 0.5 if spec.get("long_reads") else 0.3
keep, absolute, met, info, passed, _, _ = eng.profile_step(avg, fr=fr)
hap_off = eng.hap_off.astype(np.int64)
off, hap, w = [0], [], []
for s in range(eng.S):
    for h in range(hap_off[s], hap_off[s + 1]):
        if passed[h]:
            hap.append(h - hap_off[s])
            w.append(met[h].second_sol)
    off.append(len(hap))
cands = (np.array(off, dtype=np.uint64), np.array(hap, dtype=np.uint32), np.array(w, dtype=np.float64))
R, T = rd.n_reads, len(rd.node_id)
K = np.diff(cands[0].astype(np.int64))
print("reported: %d over %d species (widest list %d)" % (len(hap), eng.S, int(K.max())), flush=True)
# The keys of a paired-end sample.  The generator shuffles its reads, so neighbours in the file sit in different species (pairing 2i with 2i + 1 leaves
# 0.998 of the reads in mate_elsewhere and the join idle); the reads are paired within the species of their first node instead: in the stable order by
# species, positions 2j and 2j + 1 share key splitmix64(j) and carry the tags 1 and 2.  The last read of an odd R stays single.
so = rd.step_off.astype(np.int64)
first = rd.node_id[np.minimum(so[:-1], len(rd.node_id) - 1)].astype(np.int64)
starts = np.array([g.range_start for g in species], dtype=np.int64)
order = np.argsort(np.searchsorted(starts, first, side="right"), kind="stable")
j = np.arange(R, dtype=np.uint64)
z = (j >> np.uint64(1)) + np.uint64(0x9E3779B97F4A7C15)
z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
key, tag = np.zeros(R, dtype=np.uint64), np.zeros(R, dtype=np.uint8)
key[order] = z ^ (z >> np.uint64(31))
tag[order] = ((j & np.uint64(1)) + np.uint64(1)).astype(np.uint8)
want_mate = np.full(R, 0xFFFFFFFF, dtype=np.uint32)
even = R - R % 2
want_mate[order[0:even:2]] = order[1:even:2]
want_mate[order[1:even:2]] = order[0:even:2]
del so, first, j, z


def timed(call):
    out = call()                                                  # warm-up
    eng.timing_enable(True)
    eng.timing_reset()
    t0 = time.perf_counter()
    for _ in range(N):
        out = call()
    wall = (time.perf_counter() - t0) / N
    rows = eng.timing_get()
    eng.timing_enable(False)
    return out, wall * 1e3, {k: ms / N for k, (launches, ms) in rows.items()}


sup, sup_wall, sup_ms = timed(lambda: eng.strain_read_support(*cands))
(mate, counts), mt_wall, mt_ms = timed(lambda: eng.fragment_mates(key, tag))
assert int(counts[0]) == R // 2 and int(counts[2]) == 0 and np.array_equal(mate, want_mate), "the pairs are the ones that were named"
frg, fr_wall, fr_ms = timed(lambda: eng.strain_fragments(*cands, mate))
f_hap, f_species, status, pair_off, pair, _ = frg
sort_ms = sum(ms for k, ms in mt_ms.items() if k.startswith("sort_"))
res = {"workload": name, "reads": R, "steps": T, "reported": len(hap), "species": eng.S, "skipped_species": int((K > 64).sum()),
       "sort_ms": sort_ms, "frag_iota_kernel_ms": mt_ms.get("frag_iota_kernel", 0.0), "frag_pair_kernel_ms": mt_ms.get("frag_pair_kernel", 0.0),
       "frag_mate_slot_kernel_ms": fr_ms.get("frag_mate_slot_kernel", 0.0), "frag_mask_kernel_ms": fr_ms.get("frag_mask_kernel", 0.0),
       "frag_join_kernel_ms": fr_ms.get("frag_join_kernel", 0.0), "read_support_kernel_ms": sup_ms.get("read_support_kernel", 0.0),
       "fragment_mates_call_ms_wall": mt_wall, "strain_fragments_call_ms_wall": fr_wall, "strain_read_support_call_ms_wall": sup_wall,
       "mates_kernels": {k: v for k, v in mt_ms.items()}, "fragments_kernels": {k: v for k, v in fr_ms.items()}}
res.update({n: int(c) for n, c in zip(("counted_reads", "paired", "concordant", "discordant", "half", "unexplained", "single", "multi", "mate_elsewhere"),
                                      f_species[:, :, 0].sum(axis=0))})
res.update({n: int(c) for n, c in zip(("compatible", "unique", "unique_by_pair", "assigned"), f_hap[:, :, 0].sum(axis=0))})
assert np.array_equal(f_species[:, 0], sup[1][:, 0]), "counted differs from the read support pass"
served = status == 0
assert np.array_equal(f_species[served, 1], f_species[served, 2:6].sum(axis=1)) and int(pair.sum()) == 2 * int(f_species[served, 3, 0].sum()), "the identities of the contract"
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
