#!/usr/bin/env python3
"""Search by example rows (vdb_flat_knn_like: the average of positive rows steered away from negative rows, searched exactly, the
examples left out) against its floor and against what a caller did before, same process, same table.

1M x 960 f32 rows (bench data, seed 1806) in a VecDB table, 1000 queries, k = 10, positives per query in 1, 5, 50 and negatives in 0, 5
(random rows).  Host clock around calls that end synchronised, median of --reps (20) with the range, everything from this one run; per
(positives, negatives):
  like         vdb_flat_knn_like_device: k_like_build, the list call at K' = k + positives + negatives, k_like_drop
  build, drop  the two kernels alone, between events (vdb_prof_get "like_build" / "like_drop" of further calls with the profile on)
  floor        vdb_flat_knn_device at k = K' over the built queries, unfiltered: the list call the like call cannot beat
  host         the route the call replaces: GpuIndex.get_rows of every example, a numpy mean per query, VecDB.batch_search at K', and a
               Python drop of the examples (its query vectors are numpy's pairwise means, not the contract's strict fold)
The answers of 32 queries are compared with the floor's lists less the examples before anything is timed.  Writes one JSON record
(default profiles/flat_like_1M.json)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TIERS = ("flat_i8_queries", "flat_i8_redo", "flat_half_queries", "flat_half_redo", "flat_fallback")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--positives", type=str, default="1,5,50")
    ap.add_argument("--negatives", type=str, default="0,5")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "flat_like_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import gist_like_gpu
    from lab_1806_vec_db_amd.vecdb import VecDB

    dev = torch.device("cuda", 0)
    n, dim, k, nq = args.rows, args.dim, args.k, args.queries
    db = VecDB()
    db.create_table_if_not_exists("t", dim, "l2sqr")
    t = db._tables["t"]
    ix = t.index
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    ix.add_device(base.data_ptr(), n)  # (the rows go in from the device: a host copy of 3.84 GB is no part of what is measured)
    del base
    t.metadata = [{"id": str(i)} for i in range(n)]
    rng = np.random.default_rng(1808)

    def wall(fn, reps):
        ts, out = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": reps}, out

    rec = {"what": "search by example rows (vdb_flat_knn_like_device) against vdb_flat_knn_device at k = K' over the built queries (the floor), "
                   "k_like_build and k_like_drop alone between events, and the host route it replaces (get_rows + numpy mean + batch_search at K' "
                   "+ a Python drop); host clock around synchronised calls, medians with their ranges, one process, one table",
           "rows": n, "dim": dim, "queries": nq, "k": k, "cases": {}}

    for P in [int(x) for x in args.positives.split(",")]:
        for G in [int(x) for x in args.negatives.split(",")]:
            kp = k + P + G
            pos = rng.integers(0, n, size=(nq, P)).astype(np.uint64)
            neg = rng.integers(0, n, size=(nq, G)).astype(np.uint64)
            pl = (np.arange(nq + 1) * P).astype(np.uint64)
            nl = (np.arange(nq + 1) * G).astype(np.uint64) if G else None
            t_p = torch.from_numpy(pos.view(np.int64)).to(dev)
            t_n = torch.from_numpy(neg.view(np.int64)).to(dev) if G else None
            n_ptr = t_n.data_ptr() if G else 0
            tq = torch.zeros((nq, dim), dtype=torch.float32, device=dev)
            o_i = torch.zeros((nq, k), dtype=torch.int64, device=dev)
            o_d = torch.zeros((nq, k), dtype=torch.float32, device=dev)
            o_c = torch.zeros((nq,), dtype=torch.int64, device=dev)
            l_i = torch.zeros((nq, kp), dtype=torch.int64, device=dev)
            l_d = torch.zeros((nq, kp), dtype=torch.float32, device=dev)
            l_c = torch.zeros((nq,), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()

            def like():
                ix.flat_knn_like_device(pl, t_p.data_ptr(), nl, n_ptr, nq, k, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr())

            def floor():
                ix.flat_knn_device(tq.data_ptr(), nq, kp, l_i.data_ptr(), l_d.data_ptr(), l_c.data_ptr())

            # ---- correctness first: 32 queries against the floor's lists over the built queries, less the examples
            ix.like_queries_device(pl, t_p.data_ptr(), nl, n_ptr, nq, tq.data_ptr())
            like()
            floor()
            chk = min(32, nq)
            gi, gd, li, ld = o_i[:chk].cpu().numpy(), o_d[:chk].cpu().numpy(), l_i[:chk].cpu().numpy(), l_d[:chk].cpu().numpy()
            for q in range(chk):
                ex = set(pos[q].tolist()) | set(neg[q].tolist())
                keep = [j for j in range(kp) if int(li[q, j]) not in ex][:k]
                assert gi[q].tolist() == li[q, keep].tolist() and gd[q].tobytes() == ld[q, keep].tobytes(), (P, G, q)

            e = {"list_length": kp, "checked_queries": chk}
            s0 = {s: ix.get_stat(s) for s in TIERS}
            e["like"], _ = wall(like, args.reps)
            e["like"]["list_call_tiers_per_call"] = {s: (ix.get_stat(s) - s0[s]) / args.reps for s in TIERS}
            e["floor_flat_knn_device"], _ = wall(floor, args.reps)
            ker = {"like_build": [], "like_drop": []}
            for _ in range(5):
                ix.prof_enable(True)
                ix.prof_reset()
                like()
                for name in ker:
                    ker[name].append(ix.prof_get(name)["ms"])
                ix.prof_enable(False)
            for name, ms in ker.items():
                e[name + "_between_events"] = {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": 5}
            e["kernels_share_of_like"] = (e["like_build_between_events"]["ms_median"] + e["like_drop_between_events"]["ms_median"]) / e["like"]["ms_median"]
            e["like_over_floor"] = e["like"]["ms_median"] / e["floor_flat_knn_device"]["ms_median"]

            def host():
                rows = ix.get_rows(np.concatenate([pos.reshape(-1), neg.reshape(-1)]))
                ap = rows[:nq * P].reshape(nq, P, dim).mean(axis=1)
                qv = ap + (ap - rows[nq * P:].reshape(nq, G, dim).mean(axis=1)) if G else ap
                res = db.batch_search("t", qv.astype(np.float32), kp)
                out = []
                for q, r in enumerate(res):
                    ex = set(str(x) for x in pos[q].tolist()) | set(str(x) for x in neg[q].tolist())
                    out.append([m["id"] for m, _ in r if m["id"] not in ex][:k])
                return out

            e["host_alternative"], _ = wall(host, args.host_reps)
            e["host_over_like"] = e["host_alternative"]["ms_median"] / e["like"]["ms_median"]
            rec["cases"]["P%d_N%d" % (P, G)] = e

    rec["stats"] = {s: ix.get_stat(s) for s in ("flat_like_calls", "flat_like_queries", "like_example_rows")}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    db.delete_table("t")


if __name__ == "__main__":
    main()
