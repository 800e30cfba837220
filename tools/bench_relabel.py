#!/usr/bin/env python3
"""In-place metadata update -- the scattered label writes (vdb_index_labels_scatter, vdb_index_labels_set_mask) and
VecDB.update_metadata over them -- against the only routes the library offered before, in one process.

Default bench data (1M x 960 gist-like rows, seed 1806), L2Sqr, 1000 tenants x 1000 rows.  Measured, wall times of calls that return
synchronised, medians and min - max over the repetitions of ONE run (the first repetition of every leg warms up and is not recorded):

  GpuIndex   set_labels_mask over one tenant's mask and over a 10 % mask; set_labels_rows over a shuffled 0.1 %, 1 % and 10 % of the rows
             with 1 and 3 columns; each list against the parent's only library route for scattered rows: labels_get of the whole
             column, a patch on the host, labels_set of the whole column, per column
  VecDB      update_metadata of one tenant's rows against delete + batch_add of the same rows (same vectors) on a twin table; then
             batch_search over all tenant filters right after an update_metadata on ANOTHER key (the tenant masks stay: expected 0
             built), right after one on `tenant` itself (they are rebuilt) and right after the delete + batch_add route

No test asserts any of these times.  Writes one JSON record (default profiles/relabel_1M.json)."""
from __future__ import annotations

import argparse
import gc
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
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tenants", type=int, default=1000)
    ap.add_argument("--no-vecdb", action="store_true", help="skip the VecDB part")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "relabel_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    import lab_1806_vec_db_amd as vdb
    from bench import gist_like_gpu

    dev = torch.device("cuda", 0)
    n, dim, k, T = args.rows, args.dim, args.k, args.tenants
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    rng = np.random.default_rng(1811)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def summary(ts):
        ts = ts[1:]  # (the first repetition warms the leg up)
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": len(ts)}

    # ---- GpuIndex: the library calls --------------------------------------------------------------------------------------------------
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.add_device(base.data_ptr(), n)
    tenant = (np.arange(n) % T).astype(np.uint32)
    for c in range(3):
        ix.set_labels(c, tenant if c == 0 else rng.integers(0, 50, size=n).astype(np.uint32))
    ix.prof_enable(True)

    def parent_route(rows, cols, codes):
        for c, col in enumerate(cols):
            whole = ix.get_labels(col)
            whole[rows] = codes[c]
            ix.set_labels(col, whole)

    cases = []
    one = ix.make_mask_where([(0, 17)])
    tenth = ix.make_mask(np.sort(rng.choice(n, n // 10, replace=False)))
    for name, mk in (("one tenant's mask", one), ("10 % mask", tenth)):
        for n_cols in (1, 3):
            cols = [1, 2, 0][:n_cols]
            ts = [wall(lambda: ix.set_labels_mask(mk, cols, [rep + 60] * n_cols)) for rep in range(args.reps + 1)]
            rec = {"call": "set_labels_mask", "set": name, "rows": len(mk), "columns": n_cols, **summary(ts)}
            cases.append(rec)
            print(json.dumps(rec), flush=True)
        ix.set_labels(0, tenant)
    for f in (0.001, 0.01, 0.1):
        for n_cols in (1, 3):
            cols = [1, 2, 0][:n_cols]
            new, old = [], []
            for rep in range(args.reps + 1):
                rows = rng.permutation(n)[:int(n * f)]
                codes = rng.integers(0, 50, size=(n_cols, len(rows))).astype(np.uint32)
                new.append(wall(lambda: ix.set_labels_rows(rows, cols, codes)))
                old.append(wall(lambda: parent_route(rows, cols, codes)))
            rec = {"call": "set_labels_rows", "set": f"shuffled {100 * f:g} %", "rows": int(n * f), "columns": n_cols, **summary(new),
                   "parent_get_patch_set": summary(old)}
            rec["parent_over_call"] = rec["parent_get_patch_set"]["ms_median"] / rec["ms_median"]
            cases.append(rec)
            print(json.dumps(rec), flush=True)
    prof = ix.prof_get("labels_scatter")
    ms, launches = prof["ms"], prof["launches"]
    out = {
        "what": "scattered label writes: GpuIndex.set_labels_mask / set_labels_rows (one launch per call) vs labels_get + host patch + labels_set "
                "of the whole column, per column; wall times of calls that return synchronised, Python layer included; medians and ranges over "
                "the repetitions of ONE run",
        "rows": n, "dim": dim, "tenants": T, "cases": cases,
        "kernels": {"labels_scatter_ms_total": ms, "launches": int(launches), "ms_per_launch": ms / max(int(launches), 1)},
        "stats": {s: ix.get_stat(s) for s in ("labels_scatter_calls", "labels_scatter_rows", "labels_scatter_span")},
    }
    for mk in (one, tenth):
        mk.close()
    ix.close()

    # ---- VecDB ------------------------------------------------------------------------------------------------------------------------------
    if not args.no_vecdb:
        from lab_1806_vec_db_amd.vecdb import VecDB

        tq = gist_like_gpu(torch, T, dim, 1808, dev).cpu().numpy()
        pats = [{"tenant": str(j)} for j in range(T)]
        dbs = []
        for _ in range(2):
            db = VecDB()
            db.create_table_if_not_exists("t", dim, "l2sqr")
            t = db._tables["t"]
            t.index.add_device(base.data_ptr(), n)  # (the rows go in from the device: a host copy of them is no part of what is measured)
            t.metadata = [{"id": str(i), "tenant": str(i % T), "year": str(2000 + i % 20)} for i in range(n)]
            db.batch_search("t", tq, k, filters=pats)  # columns, masks, mirrors
            db.count("t", {"year": "2001"})  # `year` has a column too
            db.batch_search("t", tq, k, filters=pats)
            dbs.append(db)
        del base
        # two million metadata dicts: a full pass of Python's cyclic collector over them falls on whichever call allocates at the wrong
        # moment (a run without this had 90 - 100 ms outliers among searches of 10 - 17 ms, which such a pass would explain); they are
        # taken out of the collector's view
        gc.collect()
        gc.freeze()
        db_u, db_p = dbs
        mstats = ("mask_where_masks", "mask_partition_masks")

        def built(db):
            return sum(db._tables["t"].index.get_stat(s) for s in mstats)

        legs = {name: [] for name in ("update_metadata_other_key", "search_after_update_other_key", "update_metadata_tenant", "search_after_update_tenant",
                                      "delete_and_batch_add", "search_after_delete_and_batch_add", "search_warm")}
        masks_built = {"after_update_other_key": 0, "after_update_tenant": 0, "after_delete_and_batch_add": 0}
        for rep in range(args.reps + 1):
            w = str((rep * 37) % T)
            legs["search_warm"].append(wall(lambda: db_u.batch_search("t", tq, k, filters=pats)))
            legs["update_metadata_other_key"].append(wall(lambda: db_u.update_metadata("t", {"tenant": w}, {"year": f"r{rep}"})))
            b0 = built(db_u)
            legs["search_after_update_other_key"].append(wall(lambda: db_u.batch_search("t", tq, k, filters=pats)))
            masks_built["after_update_other_key"] += (built(db_u) - b0) if rep else 0
            # (the value it has: the table stays as it was, the write on `tenant` still drops the tenant masks)
            legs["update_metadata_tenant"].append(wall(lambda: db_u.update_metadata("t", {"tenant": w}, {"tenant": w})))
            b0 = built(db_u)
            legs["search_after_update_tenant"].append(wall(lambda: db_u.batch_search("t", tq, k, filters=pats)))
            masks_built["after_update_tenant"] += (built(db_u) - b0) if rep else 0
            vecs, meta = db_p.get("t", {"tenant": w})  # (not timed: the parent's route needs the vectors back)
            meta = [dict(m, year=f"r{rep}") for m in meta]

            def parent():
                db_p.delete("t", {"tenant": w})
                db_p.batch_add("t", vecs, meta)

            legs["delete_and_batch_add"].append(wall(parent))
            b0 = built(db_p)
            legs["search_after_delete_and_batch_add"].append(wall(lambda: db_p.batch_search("t", tq, k, filters=pats)))
            masks_built["after_delete_and_batch_add"] += (built(db_p) - b0) if rep else 0
        out["vecdb"] = {
            "what": f"VecDB.update_metadata of one tenant's {n // T} rows (a change of `year`, then a write of `tenant`) vs delete + batch_add of the same "
                    f"rows on a twin table, and VecDB.batch_search, one query per tenant, all {T} tenant filters, right after each; 'search_warm' = "
                    "the same search with nothing written before it",
            "tenants": T, "rows_per_tenant": n // T,
            **{name: summary(ts) for name, ts in legs.items()},
            "masks_built_by_the_searches": masks_built,
            "stats": {s: db_u._tables["t"].index.get_stat(s) for s in ("labels_scatter_calls", "labels_scatter_rows")},
        }
        for db in dbs:
            db.delete_table("t")
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
