#!/usr/bin/env python3
"""Measurement: the pairwise strain distinguishability of a db (pantax_hip_db_hap_pairs) on a bench workload.  Builds the set as bench.py does, uploads
the db -- no reads, no step: the call needs nothing else --, selects every haplotype of every species and times the node pass through timing_get: ms per
kernel variant (hap_pairs_kernel<8 | 16 | 32 | 64>, by the columns a wave keeps), algorithmic bytes and the fraction of 8 TB/s.  With route "walk" the
membership comes from the selected walks (hap_pairs_route=walk): the mask pass is timed too.
usage: hap_pairs_probe.py [workload (cfg4)] [repeats (3)] [route (node | walk)] [record.json]"""
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
route = sys.argv[3] if len(sys.argv) > 3 else "node"
record = sys.argv[4] if len(sys.argv) > 4 else None
spec = bench.workload_spec(name)
t0 = time.perf_counter()
ns = bench.native_set(spec, threads=min(16, os.cpu_count() or 1))
species = ns.graphs()
print("%s: %d species generated in %.1f s" % (name, len(species), time.perf_counter() - t0), flush=True)
eng = Engine(0)
eng.upload_db(species)
K = np.array([g.n_paths for g in species], dtype=np.int64)
sel = (np.concatenate([[0], np.cumsum(K)]).astype(np.uint64), np.concatenate([np.arange(k, dtype=np.uint32) for k in K]))
V = int(eng.node_off[-1])
p_sel = int(sum(int(g.path_off[-1]) for g in species))
nw = (K + 63) // 64
by_node = route != "walk"
words = np.where((K <= 64) & by_node, 1, nw)                      # mask words per node: the node -> haplotype word of route 1, the compact masks of route 2
tiles = words * (words + 1) // 2                                  # block pairs of every species
nodes = np.array([g.n_nodes for g in species], dtype=np.int64)
# one node read per block pair: 4 (length) + 8 a word, two words off the diagonal; + every word once more for m(v) where a species has several
b_node = int((nodes * (words * 12 + (tiles - words) * 20 + np.where(words > 1, 8 * words, 0))).sum())
print("selected: %d haplotypes over %d species (K %d .. %d), %d nodes, %d path steps, %d pair entries" % (int(K.sum()), eng.S, K.min(), K.max(), V, p_sel, int((K * K).sum())), flush=True)
if route == "walk":
    eng.set_option("hap_pairs_route", "walk")
out = eng.hap_pairs(sel[0], sel[1])                                # warm-up
eng.timing_enable(True)
eng.timing_reset()
t0 = time.perf_counter()
for _ in range(N):
    out = eng.hap_pairs(sel[0], sel[1])
wall = (time.perf_counter() - t0) / N
rows = eng.timing_get()
eng.timing_enable(False)
eng.set_option("hap_pairs_route", None)
per = lambda k: rows.get(k, (0, 0.0))[1] / max(N, 1)
variants = {k: per(k) for k in sorted(rows) if k.startswith("hap_pairs_kernel")}
ms_node, ms_mask = sum(variants.values()), per("read_strain_mask_kernel")
pair_off, pair, sp = out
po = pair_off.astype(np.int64)
ident = nested = 0
min_dist = []
for s in range(eng.S):
    P = pair[po[s]:po[s + 1], 1].reshape(K[s], K[s]).astype(np.int64)
    d = np.diag(P)
    only_a, only_b = d[:, None] - P, d[None, :] - P
    up = np.triu(np.ones_like(P, dtype=bool), 1)
    ident += int(((only_a == 0) & (only_b == 0) & up).sum())
    nested += int((((only_a == 0) ^ (only_b == 0)) & up).sum())
    if up.any():
        min_dist.append(int((only_a + only_b)[up].min()))
res = {"workload": name, "route": route, "repeats": N, "haplotypes": int(K.sum()), "species": eng.S, "nodes": V, "pair_entries": int((K * K).sum()),
       "call_ms_wall": wall * 1e3, "hap_pairs_kernel_ms": ms_node, "hap_pairs_kernel_ms_by_columns": variants, "hap_pairs_kernel_gb": b_node / 1e9,
       "hap_pairs_kernel_of_8TBs": b_node / ms_node / 1e6 / 8000 if ms_node else None,
       "read_strain_mask_kernel_ms": ms_mask if route == "walk" else None, "selected_path_steps": p_sel,
       "core_nodes": int(sp[:, 2, 0].sum()), "none_nodes": int(sp[:, 1, 0].sum()), "total_len": int(sp[:, 0, 1].sum()),
       "identical_pairs": ident, "nested_pairs": nested, "smallest_distance_median_over_species": float(np.median(min_dist)) if min_dist else None}
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
