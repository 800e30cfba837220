#!/usr/bin/env python3
"""Filtered Flat k-NN with one mask per query (vdb_flat_knn_filtered_multi_device) against the loop of single-mask calls that served
such a batch before, and against the unfiltered call, same process, same queries, legs alternating.

1M x 960 gist-like rows (the default bench data, seeds 1806 / 1807), k = 10, 1000 queries per step.  Shapes:
  (a) 1000 tenants of 1000 rows each, disjoint; one query per tenant             -- grouped path
  (b) the first 125 of those tenants, 8 queries each                             -- grouped path
  (c) 8 tenants of 125 000 rows, 125 queries each                                -- the long-mask route (8-bit tier per mask)
Legs per shape: `multi` = ONE multi call; `loop` = one vdb_flat_knn_filtered_device call per tenant over that tenant's queries (the
queries are laid out tenant after tenant, so the loop needs no gather); `knn` = the unfiltered 1000-query call.  Device events around
calls that end synchronised; WARMUP + STEPS steps; median, min and max per leg.  For (a) and (b) the grouped kernel's bytes over its
time (vdb_prof_get "flat_filtered_scan_grouped", from a separate profiled pass) are reported as a fraction of vdb_stream_probe on this
box.  Writes one JSON record (default profiles/flat_filtered_multi_1M.json)."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FSTATS = ("flat_filtered_queries", "flat_filtered_direct_queries", "flat_filtered_i8_queries", "flat_filtered_fallback_queries",
          "flat_filtered_multi_calls", "flat_filtered_grouped_queries")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--dist", choices=["l2sqr", "cosine"], default="l2sqr")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", type=str, default="a,b,c")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "flat_filtered_multi_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    import lab_1806_vec_db_amd as vdb
    from bench import gist_like_gpu
    from lab_1806_vec_db_amd.index import stream_probe

    dev = torch.device("cuda", 0)
    n, dim, nq, k = args.rows, args.dim, args.nq, args.k
    probe_gbps = stream_probe(0)
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    qs = gist_like_gpu(torch, nq, dim, 1807, dev)
    ix = vdb.GpuIndex(dim, args.dist)
    ix.add_device(base.data_ptr(), n)
    del base
    oi = torch.zeros(nq, k, dtype=torch.int64, device=dev)
    od = torch.zeros(nq, k, device=dev)
    oc = torch.zeros(nq, dtype=torch.int64, device=dev)
    perm = np.random.default_rng(1808).permutation(n)  # tenants are random disjoint row sets

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def knn_step():
        return timed(lambda: ix.flat_knn_device(qs.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr()))

    def shape(tenants, rows_each, per_tenant):
        masks = [ix.make_mask(perm[t * rows_each:(t + 1) * rows_each]) for t in range(tenants)]
        mask_of = np.repeat(np.arange(tenants, dtype=np.uint32), per_tenant)  # tenant after tenant: the loop's blocks are contiguous
        assert len(mask_of) == nq
        return masks, mask_of, per_tenant

    shapes = {
        "a": lambda: shape(nq, n // nq, 1),
        "b": lambda: shape(nq // 8, n // nq, 8),
        "c": lambda: shape(8, n // 8, nq // 8),
    }
    cases = []
    for name in args.shapes.split(","):
        masks, mask_of, per = shapes[name]()

        def multi_step():
            return timed(lambda: ix.flat_knn_filtered_multi_device(qs.data_ptr(), nq, k, masks, mask_of, oi.data_ptr(), od.data_ptr(), oc.data_ptr()))

        def loop_step():
            def run():
                for t, mk in enumerate(masks):
                    o = t * per
                    ix.flat_knn_filtered_device(qs.data_ptr() + o * dim * 4, per, k, mk, oi.data_ptr() + o * k * 8, od.data_ptr() + o * k * 4,
                                                oc.data_ptr() + o * 8)
            return timed(run)

        # the two filtered legs agree (bits) before anything is timed
        multi_step()
        ref = (oi.clone(), od.clone(), oc.clone())
        loop_step()
        assert torch.equal(ref[0], oi) and torch.equal(ref[1].view(torch.int32), od.view(torch.int32)) and torch.equal(ref[2], oc), name
        for _ in range(args.warmup):
            multi_step(), loop_step(), knn_step()
        s0 = {s: ix.get_stat(s) for s in FSTATS}
        tm, tl, tk = [], [], []
        for _ in range(args.steps):
            tm.append(multi_step())
            tl.append(loop_step())
            tk.append(knn_step())
        d = {s: (ix.get_stat(s) - s0[s]) / args.steps for s in FSTATS}
        row = {"shape": name, "tenants": len(masks), "rows_per_tenant": len(masks[0]), "queries_per_tenant": per}
        for leg, t in (("multi", tm), ("loop", tl), ("knn", tk)):
            row[f"{leg}_step_ms_median"], row[f"{leg}_step_ms_min"], row[f"{leg}_step_ms_max"] = float(np.median(t)), float(np.min(t)), float(np.max(t))
        row["loop_over_multi"] = row["loop_step_ms_median"] / row["multi_step_ms_median"]
        row["multi_over_knn"] = row["multi_step_ms_median"] / row["knn_step_ms_median"]
        row["per_step_counters_multi_plus_loop"] = d
        # the grouped kernel alone, from a profiled pass of its own (event pairs inside the call)
        ix.prof_enable(True)
        ix.prof_reset()
        for _ in range(3):
            multi_step()
        p = ix.prof_get("flat_filtered_scan_grouped")
        ix.prof_enable(False)
        if p["launches"]:
            gbps = p["bytes"] / (p["ms"] * 1e-3) / 1e9
            row["grouped_scan"] = {"launches": p["launches"], "ms_per_launch": p["ms"] / p["launches"], "gbytes_per_launch": p["bytes"] / p["launches"] / 1e9,
                                   "gbps": gbps, "fraction_of_stream_probe": gbps / probe_gbps}
        cases.append(row)
        print(json.dumps(row), flush=True)
        for mk in masks:
            mk.close()
    rec = {
        "what": "filtered Flat k-NN with one mask per query (vdb_flat_knn_filtered_multi_device) vs the loop of vdb_flat_knn_filtered_device calls over "
                "the same masks vs vdb_flat_knn_device, same process, alternating legs, device events around synchronised calls",
        "rows": n, "dim": dim, "nq": nq, "dist": args.dist, "k": k, "steps": args.steps, "warmup": args.warmup,
        "stream_probe_gbps": probe_gbps, "cases": cases,
    }
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
