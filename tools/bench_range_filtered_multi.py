#!/usr/bin/env python3
"""Filtered Flat range search with one mask per query (vdb_flat_range_filtered_multi) against the loop of vdb_flat_range_filtered calls
that served such a batch before, and against the grouped k-NN call at k = 64, same process, same queries, legs alternating.

1M x 960 gist-like rows (the default bench data, seeds 1806 / 1807), 1000 queries per step, radius of a query = its own 64th allowed
distance (so every slice holds 64 pairs, more on a tie).  Shapes:
  (a) 1000 tenants of 1000 rows each, disjoint; one query per tenant             -- grouped path
  (b) the first 125 of those tenants, 8 queries each                             -- grouped path
  (c) 8 tenants of 125 000 rows, 125 queries each                                -- the per-mask route
Legs per shape: `multi` = ONE vdb_flat_range_filtered_multi call (host queries and radii, like the loop's calls); `multi_device` = the
_device form; `loop` = one vdb_flat_range_filtered call per tenant over that tenant's queries (the queries are laid out tenant after
tenant, so the loop needs no gather); `knn` = vdb_flat_knn_filtered_multi_device at k = 64 over the same batch.  With --loop-calls N
the loop leg times its first N calls only and the record says so (the figure is then scaled to the whole loop).  Device events around
calls that end synchronised; WARMUP + STEPS steps; median, min and max per leg; the range legs' results are compared bit for bit before
anything is timed.  For the shapes on the grouped path the grouped kernel's bytes over its time (vdb_prof_get
"flat_range_gather_grouped", from a separate profiled pass) are reported as a fraction of vdb_stream_probe on this box.

The sweep (--sweep): 8 masks of m rows (random row sets, disjoint while 8 m <= rows) with 8 queries each, m in powers of two from 1024 to
262144, answered once with flat_filtered_direct_max raised to m (grouped path) and once with it at 0 (per-mask route) -- where the
crossover between the two lies for the RANGE call.  Writes one JSON record (default profiles/flat_range_filtered_multi_1M.json)."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RSTATS = ("flat_range_queries", "flat_range_i8_queries", "flat_range_scan_queries", "flat_range_results", "flat_range_multi_calls",
          "flat_range_grouped_queries")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--rank", type=int, default=64, help="the radius of a query is its rank-th allowed distance")
    ap.add_argument("--dist", choices=["l2sqr", "cosine"], default="l2sqr")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", type=str, default="a,b,c", help="'' = none")
    ap.add_argument("--loop-calls", type=int, default=0, help="time only the first N calls of the loop leg (0: all)")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "flat_range_filtered_multi_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    import lab_1806_vec_db_amd as vdb
    from bench import gist_like_gpu
    from lab_1806_vec_db_amd.index import stream_probe

    dev = torch.device("cuda", 0)
    n, dim, nq, rank = args.rows, args.dim, args.nq, args.rank
    probe_gbps = stream_probe(0)
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    qs = gist_like_gpu(torch, nq, dim, 1807, dev)
    ix = vdb.GpuIndex(dim, args.dist)
    ix.add_device(base.data_ptr(), n)
    del base
    h_qs = qs.cpu().numpy()
    oi = torch.zeros(nq, rank, dtype=torch.int64, device=dev)
    od = torch.zeros(nq, rank, device=dev)
    oc = torch.zeros(nq, dtype=torch.int64, device=dev)
    perm = np.random.default_rng(1808).permutation(n)  # tenants are random disjoint row sets

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def summary(row, leg, t):
        row[f"{leg}_step_ms_median"], row[f"{leg}_step_ms_min"], row[f"{leg}_step_ms_max"] = float(np.median(t)), float(np.min(t)), float(np.max(t))

    def same(x, y):
        return all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
                   for a, b in zip(x, y))

    def radii_of(q, nqs, masks, mask_of):
        """per query its rank-th allowed distance, from the grouped k-NN call (device tensor and host array)"""
        ix.flat_knn_filtered_multi_device(q.data_ptr(), nqs, rank, masks, mask_of, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        assert int(oc[:nqs].min()) == rank
        r = od[:nqs, rank - 1].contiguous()
        return r, r.cpu().numpy()

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
    for name in [s for s in args.shapes.split(",") if s]:
        masks, mask_of, per = shapes[name]()
        d_r, h_r = radii_of(qs, nq, masks, mask_of)
        calls = len(masks) if args.loop_calls <= 0 else min(args.loop_calls, len(masks))

        def multi_step():
            return timed(lambda: ix.range_search_multi(h_qs, h_r, masks, mask_of))

        def multi_device_step():
            return timed(lambda: ix.range_search_multi_device(qs.data_ptr(), nq, d_r.data_ptr(), masks, mask_of))

        def loop_step(ncalls):
            def run():
                return [ix.range_search(h_qs[t * per:(t + 1) * per], h_r[t * per:(t + 1) * per], mask=masks[t]) for t in range(ncalls)]
            return timed(run)

        def knn_step():
            return timed(lambda: ix.flat_knn_filtered_multi_device(qs.data_ptr(), nq, rank, masks, mask_of, oi.data_ptr(), od.data_ptr(), oc.data_ptr()))[0]

        # the range legs agree (bits) before anything is timed
        _, ref = multi_step()
        _, refd = multi_device_step()
        assert same(ref, refd), name
        assert int(np.diff(ref[0].astype(np.int64)).min()) >= rank
        _, parts = loop_step(calls)
        cut = int(ref[0][calls * per])
        assert same((np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])), (ref[1][:cut], ref[2][:cut])), name
        assert np.array_equal(np.concatenate([np.diff(p[0].astype(np.int64)) for p in parts]), np.diff(ref[0].astype(np.int64))[:calls * per]), name
        for _ in range(args.warmup):
            multi_step(), multi_device_step(), loop_step(calls), knn_step()
        s0 = {s: ix.get_stat(s) for s in RSTATS}
        tm, td, tl, tk = [], [], [], []
        for _ in range(args.steps):
            tm.append(multi_step()[0])
            td.append(multi_device_step()[0])
            tl.append(loop_step(calls)[0] * len(masks) / calls)
            tk.append(knn_step())
        d = {s: (ix.get_stat(s) - s0[s]) / args.steps for s in RSTATS}
        row = {"shape": name, "tenants": len(masks), "rows_per_tenant": len(masks[0]), "queries_per_tenant": per, "pairs_per_step": int(ref[0][-1]),
               "loop_calls_timed": calls, "loop_extrapolated": calls != len(masks)}
        for leg, t in (("multi", tm), ("multi_device", td), ("loop", tl), ("knn_k64", tk)):
            summary(row, leg, t)
        row["loop_over_multi"] = row["loop_step_ms_median"] / row["multi_step_ms_median"]
        row["multi_over_knn_k64"] = row["multi_device_step_ms_median"] / row["knn_k64_step_ms_median"]
        row["per_step_counters_all_range_legs"] = d
        # the grouped kernel alone, from a profiled pass of its own (event pairs inside the call)
        ix.prof_enable(True)
        ix.prof_reset()
        for _ in range(3):
            multi_device_step()
        p = ix.prof_get("flat_range_gather_grouped")
        ix.prof_enable(False)
        if p["launches"]:
            gbps = p["bytes"] / (p["ms"] * 1e-3) / 1e9
            row["grouped_kernel"] = {"launches": p["launches"], "ms_per_launch": p["ms"] / p["launches"], "gbytes_per_launch": p["bytes"] / p["launches"] / 1e9,
                                     "gbps": gbps, "fraction_of_stream_probe": gbps / probe_gbps}
        cases.append(row)
        print(json.dumps(row), flush=True)
        for mk in masks:
            mk.close()

    sweep = []
    if args.sweep:
        sq, n_masks, per = 64, 8, 8
        q64 = qs[:sq].contiguous()
        mask_of = np.repeat(np.arange(n_masks, dtype=np.uint32), per)
        m = 1024
        while m <= 262144 and m <= n:
            # windows of the permutation n / 8 apart: disjoint up to m = n / 8, overlapping beyond
            masks = [ix.make_mask(perm[(np.arange(m) + t * (n // n_masks)) % n]) for t in range(n_masks)]
            ix.set_param("flat_filtered_direct_max", 8192)
            d_r, _ = radii_of(q64, sq, masks, mask_of)
            row = {"m": m, "masks": n_masks, "queries_per_mask": per}
            legs = (("grouped", m), ("per_mask", 0))
            res, times = {}, {leg: [] for leg, _ in legs}
            for step in range(args.warmup + args.steps):
                for leg, direct_max in legs:
                    ix.set_param("flat_filtered_direct_max", direct_max)
                    s0 = ix.get_stat("flat_range_grouped_queries")
                    t, out = timed(lambda: ix.range_search_multi_device(q64.data_ptr(), sq, d_r.data_ptr(), masks, mask_of))
                    assert ix.get_stat("flat_range_grouped_queries") - s0 == (sq if leg == "grouped" else 0)
                    res[leg] = out
                    if step >= args.warmup:
                        times[leg].append(t)
                assert same(res["grouped"], res["per_mask"]), m
            for leg, _ in legs:
                summary(row, leg, times[leg])
            row["per_mask_over_grouped"] = row["per_mask_step_ms_median"] / row["grouped_step_ms_median"]
            sweep.append(row)
            print(json.dumps(row), flush=True)
            for mk in masks:
                mk.close()
            m *= 2
        ix.set_param("flat_filtered_direct_max", 8192)

    rec = {
        "what": "filtered Flat range search with one mask per query (vdb_flat_range_filtered_multi / _device) vs the loop of vdb_flat_range_filtered "
                "calls over the same masks vs vdb_flat_knn_filtered_multi_device at k = 64, same process, alternating legs, device events around "
                "synchronised calls; sweep: grouped path (flat_filtered_direct_max = m) vs per-mask route (= 0), 8 masks x 8 queries",
        "rows": n, "dim": dim, "nq": nq, "dist": args.dist, "radius_rank": rank, "steps": args.steps, "warmup": args.warmup,
        "stream_probe_gbps": probe_gbps, "cases": cases, "sweep": sweep,
    }
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    ix.close()


if __name__ == "__main__":
    main()
