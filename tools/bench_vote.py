#!/usr/bin/env python3
"""k-NN label vote (vdb_flat_knn_vote_device: the exact list of k rows per query + k_vote_lists) against its floor, vdb_flat_knn_device at
the same k in the same run -- the vote runs that very list call and one kernel behind it, which is expected to be well under 1 % of the
call -- and against the host route: VecDB.batch_search at k, one dict(metadata) per hit and a collections.Counter per query.

1M x 960 f32 rows (bench data, seed 1806) with a `tenant` column (1000 values, row % 1000) and a `doc` column (10 rows per value), 1000
queries, k = 10 / 40 / 128, uniform and inverse-distance weights, top 3.  Median of --reps calls, host clock around synchronised calls;
one further call with the profile on for the kernel between events (prof_get "vote_lists").  The top value of the uniform vote is compared
with the Counter's for every query whose Counter has no tie at the top.  Not measured: masks, Cosine, u8 rows, k past 1024 (the scratch
table), other top sizes.  Nothing is gated on these numbers.  Writes --out as JSON."""
import argparse
import collections
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COLUMNS = {"tenant": 0, "doc": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "flat_vote_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import gist_like_gpu
    from lab_1806_vec_db_amd.vecdb import VecDB

    dev = torch.device("cuda", 0)
    n, dim, nq, top = args.rows, args.dim, args.queries, 3
    db = VecDB()
    db.create_table_if_not_exists("t", dim, "l2sqr")
    t = db._tables["t"]
    ix = t.index
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    ix.add_device(base.data_ptr(), n)  # (the rows go in from the device: a host copy of 3.84 GB is no part of what is measured)
    del base
    codes = {"tenant": (np.arange(n) % 1000).astype(np.uint32), "doc": (np.arange(n) // 10).astype(np.uint32)}
    for f, c in COLUMNS.items():
        ix.set_labels(c, codes[f])
    t.metadata = [{"id": str(i), "tenant": str(i % 1000), "doc": str(i // 10)} for i in range(n)]
    tq = gist_like_gpu(torch, nq, dim, 1807, dev)
    hq = tq.cpu().numpy()

    def wall(fn, reps):
        ts, out = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": reps}, out

    rec = {"what": "k-NN label vote (vdb_flat_knn_vote_device) against vdb_flat_knn_device at the same k in the same run (the floor: the same "
                   "list call) and against VecDB.batch_search plus a collections.Counter per query; host clock around synchronised calls, one "
                   "process, one table", "rows": n, "dim": dim, "queries": nq, "top": top, "cases": {}}
    for k in (10, 40, 128):
        l_i = torch.zeros((nq, k), dtype=torch.int64, device=dev)
        l_d = torch.zeros((nq, k), dtype=torch.float32, device=dev)
        l_c = torch.zeros((nq,), dtype=torch.int64, device=dev)
        o = [torch.zeros((nq, top), dtype=torch.int32, device=dev), torch.zeros((nq, top), dtype=torch.float32, device=dev),
             torch.zeros((nq, top), dtype=torch.int32, device=dev), torch.zeros((nq,), dtype=torch.int64, device=dev),
             torch.zeros((nq,), dtype=torch.int64, device=dev)]
        torch.cuda.synchronize()
        floor = lambda: ix.flat_knn_device(tq.data_ptr(), nq, k, l_i.data_ptr(), l_d.data_ptr(), l_c.data_ptr())  # noqa: E731
        floor()  # warm-up: mirrors, workspace
        e = {"floor_flat_knn_device": wall(floor, args.reps)[0]}
        for field, col in COLUMNS.items():
            for mode in ("uniform", "inverse"):
                vote = lambda: ix.flat_knn_vote_device(tq.data_ptr(), nq, k, col, top, *[x.data_ptr() for x in o], mode=mode)  # noqa: E731
                vote()
                w = wall(vote, args.reps)[0]
                ix.prof_enable(True)
                ix.prof_reset()
                vote()
                w["kernel_ms"] = ix.prof_get("vote_lists")["ms"]
                ix.prof_enable(False)
                w["ratio_to_floor"] = w["ms_median"] / e["floor_flat_knn_device"]["ms_median"]
                w["kernel_share"] = w["kernel_ms"] / w["ms_median"]
                e[f"{field}_{mode}"] = w
            vote = lambda: ix.flat_knn_vote_device(tq.data_ptr(), nq, k, col, top, *[x.data_ptr() for x in o], mode="uniform")  # noqa: E731
            vote()
            got = o[0].cpu().numpy()[:, 0]

            def host():
                return [collections.Counter(dict(m)[field] for m, _ in hits).most_common(2) for hits in db.batch_search("t", hq, k)]

            hw, hres = wall(host, args.host_reps)
            clear = [q for q, mc in enumerate(hres) if len(mc) == 1 or mc[0][1] > mc[1][1]]
            same = sum(int(hres[q][0][0]) == int(got[q]) for q in clear)
            e[f"{field}_host_batch_search_counter"] = dict(hw, queries_without_a_tie_at_the_top=len(clear), of_those_the_same_top_value=same)
            assert same == len(clear), (field, k, same, len(clear))
        rec["cases"][f"k{k}"] = e
        print(json.dumps({f"k{k}": e}), flush=True)
    rec["not_measured"] = ["masks", "Cosine", "u8 rows", "k past 1024 (scratch table)", "other top sizes"]
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    ix.close()


if __name__ == "__main__":
    main()
