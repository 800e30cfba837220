#!/usr/bin/env python3
"""Bulk row removal (vdb_index_remove_rows) against the loop of vdb_index_swap_remove it replaces -- the parent's VecDB.delete path, still
in the library -- on twin indexes in one process.

Default bench data (1M x 960 gist-like rows, seed 1806), 8-bit mirror built by a first search.  Cases: random sets of 0.1 %, 1 %, 10 % and
50 % of the rows and one contiguous block of 10 %.  Per case, on a fresh pair of indexes:

  bulk leg : wall time of ONE remove_rows call (it returns synchronised), then of the first NQ-query search after it -- next to a second,
             steady search, which shows whether the first one had to rebuild a mirror -- and whether the 8-bit mirror was still valid
  loop leg : wall time of swap_remove over the same rows in descending order.  Timed in full up to 1 % of the rows; above that the first
             LOOP_CAP removals are timed and the figure is extrapolated linearly (flagged "extrapolated": true in the record)

No test asserts any of these times.  Writes one JSON record (default profiles/bulk_remove_1M.json)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--dist", choices=["l2sqr", "cosine"], default="l2sqr")
    ap.add_argument("--loop-cap", type=int, default=10_000, help="removals of the swap_remove loop that are timed when the set is above 1 %% of the rows")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "bulk_remove_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    import lab_1806_vec_db_amd as vdb
    from bench import gist_like_gpu

    dev = torch.device("cuda", 0)
    n, dim, nq, k = args.rows, args.dim, args.nq, args.k
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    qs = gist_like_gpu(torch, nq, dim, 1807, dev)
    oi = torch.zeros(nq, k, dtype=torch.int64, device=dev)
    od = torch.zeros(nq, k, device=dev)
    oc = torch.zeros(nq, dtype=torch.int64, device=dev)
    rng = np.random.default_rng(1809)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def fresh():
        ix = vdb.GpuIndex(dim, args.dist)
        ix.add_device(base.data_ptr(), n)
        search(ix)  # builds the 8-bit mirror
        search(ix)
        assert ix.get_stat("flat_i8_valid") == 1
        return ix

    def search(ix):
        return wall(lambda: ix.flat_knn_device(qs.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr()))

    sets = [(f"random {100 * f:g} %", np.sort(rng.choice(n, int(n * f), replace=False))) for f in (0.001, 0.01, 0.1, 0.5)]
    sets.append(("block 10 %", np.arange(n // 3, n // 3 + n // 10)))
    cases = []
    for name, rows in sets:
        m = len(rows)
        ix = fresh()
        steady_before = search(ix)
        t_bulk = wall(lambda: ix.remove_rows(rows))
        valid = ix.get_stat("flat_i8_valid")
        first, steady = search(ix), search(ix)
        ids_bulk = oi.cpu().numpy().copy()
        assert len(ix) == n - m
        ix.close()
        twin = fresh()
        timed = m if m <= n // 100 else min(m, args.loop_cap)
        desc = rows[::-1][:timed].tolist()

        def loop():
            for i in desc:
                twin.swap_remove(i)

        t_loop_timed = wall(loop)
        agree = None
        if timed == m:  # the same table: the same answers
            search(twin)
            agree = bool(np.array_equal(ids_bulk, oi.cpu().numpy()))
        twin.close()
        t_loop = t_loop_timed * (m / timed)
        cases.append({
            "set": name, "removed": m, "rows_after": n - m,
            "remove_rows_ms": t_bulk, "i8_mirror_valid_after": int(valid),
            "first_search_after_ms": first, "steady_search_after_ms": steady, "steady_search_before_ms": steady_before,
            "swap_remove_loop_ms": t_loop, "extrapolated": timed != m, "loop_removals_timed": timed, "loop_timed_ms": t_loop_timed,
            "loop_over_bulk": t_loop / t_bulk, "answers_equal_loop": agree,
        })
        print(json.dumps(cases[-1]), flush=True)
    rec = {
        "what": "vdb_index_remove_rows (one call) vs a loop of vdb_index_swap_remove over the same rows, twin indexes, 8-bit mirror built; wall "
                "times of calls that return synchronised; loop figures above 1 % of the rows are extrapolated from their first removals",
        "rows": n, "dim": dim, "nq": nq, "k": k, "dist": args.dist, "loop_cap": args.loop_cap, "cases": cases,
    }
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
