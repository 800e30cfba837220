#!/usr/bin/env python3
"""Grouped Flat k-NN (vdb_flat_knn_grouped: at most g hits per value of a label column) against its floor and against what a caller did
before, same process, same table.

1M x 960 f32 rows (bench data, seed 1806) in a VecDB table as tools/bench_mask_partition.py makes it: metadata per row an id, `tenant`
(1000 tenants x 1000 rows, row i belongs to tenant i % 1000), `doc` (10 rows per value, row i belongs to document i // 10) and a
two-valued `tier`; one more column, set on the index directly, is SKEWED: 90 % of the rows under one value, every other row under a
value of its own.  Host clock around calls that end synchronised, median of --reps (40) with the range, everything from this one run:
  floor        vdb_flat_knn_device, unfiltered, the same queries and k: what the grouped call costs when nothing is capped and no list
               is lengthened
  grouped      vdb_flat_knn_grouped_device at k, g = 1, 2 and unlimited on `doc`, `tenant` and the skewed column; rounds per query
               and exhausted queries from the counters, the walk's own time from vdb_prof_get "group_cap"
  host         what a caller did before: VecDB.batch_search at K' = k x oversample and a Python walk over the returned metadata
               (one guess: queries whose K' rows keep fewer than k would need another search on top; their number is reported)
  list calls   vdb_flat_knn_device alone at K' = 10 .. 640 for all queries, before and after the sweeps, with the counters of its tiers: a
               round costs what its list call costs, and that call changes tier with K' (8-bit first pass up to 64, fp16 / split-bf16
               shortlist up to K' = 512, the exact scan beyond) and with the auto-off state of the index
  oversample   "flat_grouped_oversample" 1, 2, 4, 8, 16 at g = 1 on the three columns: time and rounds; best_oversample = the value with
               the smallest median summed over the columns
  masked       the same sweep under ONE long mask ({"tier": "gold"}, half the table) for --mask-queries queries: there K' <= 64 runs the
               filtered call's 8-bit tier and K' > 64 its direct path -- the step between oversample 4 and 8 at k = 10 is that switch (the unfiltered
               call has the same step: K' > 64 leaves its 8-bit first pass)
Every grouped answer is compared with the walk of the ungrouped search's longer list before anything is timed.  Writes one JSON record
(default profiles/flat_grouped_1M.json)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GSTATS = ("flat_grouped_calls", "flat_grouped_queries", "flat_grouped_rounds", "flat_grouped_exhausted_queries")
# the unfiltered search's own counters: which of its tiers the list calls of a timed entry ran on (per call)
TIERS = ("flat_i8_queries", "flat_i8_redo", "flat_half_queries", "flat_half_redo", "flat_fallback")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--tenants", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--mask-queries", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--mask-reps", type=int, default=10)
    ap.add_argument("--sweep", type=str, default="1,2,4,8,16")
    ap.add_argument("--default-oversample", type=int, default=2, help="the library's default (restored after the sweeps; the host alternative's K')")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "flat_grouped_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import gist_like_gpu
    from lab_1806_vec_db_amd.labels import cap_groups
    from lab_1806_vec_db_amd.vecdb import VecDB

    dev = torch.device("cuda", 0)
    n, dim, T, k, nq = args.rows, args.dim, args.tenants, args.k, args.queries
    UNLIMITED = 1 << 40
    DEFAULT = args.default_oversample
    db = VecDB()
    db.create_table_if_not_exists("t", dim, "l2sqr")
    t = db._tables["t"]
    ix = t.index
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    ix.add_device(base.data_ptr(), n)  # (the rows go in from the device: a host copy of 3.84 GB is no part of what is measured)
    del base
    t.metadata = [{"id": str(i), "tenant": str(i % T), "doc": str(i // 10), "tier": "gold" if i % 2 else "free"} for i in range(n)]
    tq = gist_like_gpu(torch, nq, dim, 1807, dev)
    qs = tq.cpu().numpy()
    t.create_columns([{"tenant": "0", "doc": "0", "tier": "gold"}])
    cols = {"doc": t.codec.column_of("doc"), "tenant": t.codec.column_of("tenant"), "skewed": 8}
    rng = np.random.default_rng(1806)
    skew = np.where(rng.random(n) < 0.9, 7, 1000 + np.arange(n)).astype(np.uint32)
    ix.set_labels(cols["skewed"], skew)
    host_labels = {"doc": ix.get_labels(cols["doc"]), "tenant": ix.get_labels(cols["tenant"]), "skewed": skew}

    def wall(fn, reps=args.reps):
        ts, out = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": reps}, out

    def outputs(m, kk):
        return (torch.zeros((m, kk), dtype=torch.int64, device=dev), torch.zeros((m, kk), dtype=torch.float32, device=dev),
                torch.zeros((m,), dtype=torch.int64, device=dev))

    o_i, o_d, o_c = outputs(nq, k)
    torch.cuda.synchronize()

    def floor():
        ix.flat_knn_device(tq.data_ptr(), nq, k, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr())

    def grouped(col, g, m=nq, masks=None):
        ix.flat_knn_grouped_device(tq.data_ptr(), m, k, col, g, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr(), masks)

    def counted(fn, reps):
        """wall() with the grouped counters of the timed calls, per query"""
        s0 = {s: ix.get_stat(s) for s in GSTATS + TIERS}
        e, _ = wall(fn, reps)
        d = {s: ix.get_stat(s) - s0[s] for s in GSTATS + TIERS}
        e["rounds_per_call"] = d["flat_grouped_rounds"] / d["flat_grouped_calls"]
        e["exhausted_queries_per_call"] = d["flat_grouped_exhausted_queries"] / d["flat_grouped_calls"]
        e["list_call_tiers_per_call"] = {s: d[s] / reps for s in TIERS}
        return e

    def list_calls():
        """vdb_flat_knn_device alone at the list lengths the rounds ask for, all queries: what a round's list call costs, and on which tiers"""
        out = {}
        for kp in (10, 20, 40, 64, 80, 160, 320, 640):
            l_i, l_d, l_c = outputs(nq, kp)
            torch.cuda.synchronize()

            def one():
                ix.flat_knn_device(tq.data_ptr(), nq, kp, l_i.data_ptr(), l_d.data_ptr(), l_c.data_ptr())

            one()
            s0 = {s: ix.get_stat(s) for s in TIERS}
            e, _ = wall(one, 10)
            e["tiers_per_call"] = {s: (ix.get_stat(s) - s0[s]) / 10 for s in TIERS}
            out[str(kp)] = e
        return out

    rec = {"what": "grouped Flat k-NN (at most g hits per value of a label column) against the unfiltered vdb_flat_knn_device at the same k (the "
                   "floor), against VecDB.batch_search at K' plus a Python walk, over flat_grouped_oversample 1..16, on a skewed column and under a "
                   "long mask; host clock around synchronised calls, medians with their ranges, one process, one table",
           "rows": n, "dim": dim, "tenants": T, "rows_per_doc": 10, "queries": nq, "k": k, "skewed_share": 0.9, "oversample_default": DEFAULT}

    # ---- correctness first: the grouped answers against the walk of the ungrouped search's longer list (64 queries)
    chk = 64
    li, ld, lc = ix.flat_knn(qs[:chk], 2048)
    for name, col in cols.items():
        for g in (1, 2):
            gi, gd, gc = ix.flat_knn_grouped(qs[:chk], k, col, g)
            for q in range(chk):
                kept = cap_groups(host_labels[name][li[q].astype(np.int64)], g, k)
                assert len(kept) == k and gi[q].tolist() == li[q][kept].tolist() and np.array_equal(gd[q], ld[q][kept]), (name, g, q)

    rec["list_call_alone_before"] = list_calls()

    # ---- the floor and the grouped call
    floor()
    rec["floor_flat_knn_device"], _ = wall(floor)
    rec["grouped"] = {}
    for name, col in cols.items():
        for g, gname in ((1, "g1"), (2, "g2"), (UNLIMITED, "unlimited")):
            grouped(col, g)
            e = counted(lambda: grouped(col, g), args.reps)
            ix.prof_enable(True)
            ix.prof_reset()
            grouped(col, g)
            p = ix.prof_get("group_cap")
            ix.prof_enable(False)
            e.update({"group_cap_ms": p["ms"], "group_cap_launches": p["launches"], "over_floor": e["ms_median"] / rec["floor_flat_knn_device"]["ms_median"]})
            rec["grouped"][f"{name}_{gname}"] = e

    # ---- what a caller did before: one search at K' and a Python walk over the metadata
    rec["host_alternative"] = {}
    for name in ("doc", "tenant"):
        for g in (1, 2):
            def host():
                short = 0
                res = db.batch_search("t", qs, DEFAULT * k)
                out = []
                for r in res:
                    kept = cap_groups([m.get(name) for m, _ in r], g, k)
                    short += len(kept) < k
                    out.append([r[p] for p in kept])
                return short

            e, short = wall(host, args.host_reps)
            e["queries_needing_another_search"] = int(short)
            e["over_grouped"] = e["ms_median"] / rec["grouped"][f"{name}_g{g}"]["ms_median"]
            rec["host_alternative"][f"{name}_g{g}"] = e

    # ---- the oversample sweep at g = 1
    sweep = [int(x) for x in args.sweep.split(",")]
    rec["oversample_sweep"] = {}
    total = {}
    for ov in sweep:
        ix.set_param("flat_grouped_oversample", ov)
        for name, col in cols.items():
            grouped(col, 1)
            e = counted(lambda: grouped(col, 1), args.reps)
            e["first_list"] = k * ov
            rec["oversample_sweep"][f"{name}_x{ov}"] = e
            total[ov] = total.get(ov, 0.0) + e["ms_median"]
    rec["best_oversample"] = min(total, key=total.get)
    rec["oversample_totals_ms"] = {str(ov): v for ov, v in total.items()}

    rec["list_call_alone_after"] = list_calls()

    # ---- the same sweep under one long mask: K' <= 64 is the filtered call's 8-bit tier, K' > 64 its direct path
    mq = min(args.mask_queries, nq)
    t.prepare([{"tier": "gold"}])
    mk = t.mask_for({"tier": "gold"})
    rec["masked_sweep"] = {"mask_rows": len(mk), "queries": mq}
    fstats = ("flat_filtered_i8_queries", "flat_filtered_direct_queries")
    for ov in sweep:
        ix.set_param("flat_grouped_oversample", ov)
        for name in ("doc", "skewed"):
            grouped(cols[name], 1, mq, mk)
            f0 = {s: ix.get_stat(s) for s in fstats}
            e = counted(lambda: grouped(cols[name], 1, mq, mk), args.mask_reps)
            e["first_list"] = k * ov
            e.update({s + "_per_call": (ix.get_stat(s) - f0[s]) / args.mask_reps for s in fstats})
            rec["masked_sweep"][f"{name}_x{ov}"] = e
    ix.set_param("flat_grouped_oversample", DEFAULT)
    rec["stats"] = {s: ix.get_stat(s) for s in GSTATS}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    db.delete_table("t")


if __name__ == "__main__":
    main()
