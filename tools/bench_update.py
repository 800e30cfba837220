#!/usr/bin/env python3
"""In-place row update (vdb_index_update_rows) against the only route the library offered before it -- remove_rows of those ids plus
batch_add of the new vectors -- on twin indexes in one process.

Default bench data (1M x 960 gist-like rows, seed 1806), L2Sqr, 8-bit mirror built by a first search.  Cases: random sets of 0.1 %, 1 %
and 10 % of the rows and one contiguous block of 10 %; new vectors from the same generator, handed over from the host.  Per case and
repetition (both indexes keep their size, so they are reused):

  update leg : wall time of ONE update_rows call (it returns synchronised), then of the first NQ-query search after it next to a second,
               steady one -- which shows whether the first had to rebuild a mirror -- and whether the 8-bit mirror was still valid
  parent leg : the same for remove_rows(ids) + batch_add(new vectors) on the twin

Then, on two VecDB tables of the same rows with 1000 tenants: VecDB.batch_search over all tenant filters right after a batch_update
(the cached masks survive) against the same search right after delete + batch_add of the same rows (the masks are rebuilt).

No test asserts any of these times.  Writes one JSON record (default profiles/update_rows_1M.json)."""
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tenants", type=int, default=1000)
    ap.add_argument("--tenants-updated", type=int, default=10)
    ap.add_argument("--no-vecdb", action="store_true", help="skip the VecDB part")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "update_rows_1M.json"), help="'' = print only")
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

    def summary(ts):
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": len(ts)}

    def search(ix):
        return wall(lambda: ix.flat_knn_device(qs.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr()))

    def fresh():
        ix = vdb.GpuIndex(dim, "l2sqr")
        ix.add_device(base.data_ptr(), n)
        search(ix)  # builds the 8-bit mirror
        search(ix)
        assert ix.get_stat("flat_i8_valid") == 1
        return ix

    ix, twin = fresh(), fresh()
    sets = [(f"random {100 * f:g} %", lambda f=f: np.sort(rng.choice(n, int(n * f), replace=False))) for f in (0.001, 0.01, 0.1)]
    sets.append(("block 10 %", lambda: np.arange(n // 3, n // 3 + n // 10)))
    cases = []
    seed = 1810
    for name, make in sets:
        legs = {"update": {"call": [], "first": [], "steady": [], "valid": []}, "parent": {"call": [], "first": [], "steady": [], "valid": []}}
        for _ in range(args.reps):
            rows = make()
            m = len(rows)
            seed += 1
            new = gist_like_gpu(torch, m, dim, seed, dev).cpu().numpy()
            for leg, x, call in (("update", ix, lambda: ix.update_rows(rows, new)),
                                 ("parent", twin, lambda: (twin.remove_rows(rows), twin.batch_add(new)))):
                before = search(x)
                legs[leg]["call"].append(wall(call))
                legs[leg]["valid"].append(int(x.get_stat("flat_i8_valid")))
                legs[leg]["first"].append(search(x))
                legs[leg]["steady"].append(search(x))
                legs[leg].setdefault("steady_before", []).append(before)
                assert len(x) == n
        rec = {"set": name, "rows_updated": m}
        for leg, d in legs.items():
            rec[leg] = {"call": summary(d["call"]), "first_search_after": summary(d["first"]), "steady_search_after": summary(d["steady"]),
                        "steady_search_before": summary(d["steady_before"]), "i8_mirror_valid_after": d["valid"]}
        rec["parent_over_update_call"] = rec["parent"]["call"]["ms_median"] / rec["update"]["call"]["ms_median"]
        cases.append(rec)
        print(json.dumps(rec), flush=True)
    out = {
        "what": "vdb_index_update_rows (one call, host vectors) vs vdb_index_remove_rows + vdb_index_add of the same rows on a twin index, "
                "8-bit mirror built; wall times of calls that return synchronised; medians and ranges over the repetitions of ONE run",
        "rows": n, "dim": dim, "nq": nq, "k": k, "dist": "l2sqr", "cases": cases,
        "stats": {s: ix.get_stat(s) for s in ("update_calls", "update_rows")},
    }
    ix.close()
    twin.close()

    if not args.no_vecdb:
        from lab_1806_vec_db_amd.vecdb import VecDB

        T, U = args.tenants, args.tenants_updated
        tq = gist_like_gpu(torch, T, dim, 1808, dev).cpu().numpy()
        pats = [{"tenant": str(j)} for j in range(T)]
        dbs = []
        for _ in range(2):
            db = VecDB()
            db.create_table_if_not_exists("t", dim, "l2sqr")
            t = db._tables["t"]
            t.index.add_device(base.data_ptr(), n)  # (the rows go in from the device: a host copy of them is no part of what is measured)
            t.metadata = [{"id": str(i), "tenant": str(i % T)} for i in range(n)]
            db.batch_search("t", tq, k, filters=pats)  # columns, masks, mirrors
            db.batch_search("t", tq, k, filters=pats)
            dbs.append(db)
        del base
        db_u, db_p = dbs
        legs = {"after_batch_update": [], "after_delete_and_batch_add": [], "warm": [], "batch_update_call": [], "delete_and_batch_add_calls": []}
        masks_built = {"after_batch_update": 0, "after_delete_and_batch_add": 0}
        mstats = ("mask_where_masks", "mask_partition_masks")

        def built(db):
            return sum(db._tables["t"].index.get_stat(s) for s in mstats)

        for rep in range(args.reps + 1):  # (the first repetition warms both routes up and is not recorded)
            who = [str((rep * U + j) % T) for j in range(U)]
            seed += 1
            vec = gist_like_gpu(torch, U, dim, seed, dev).cpu().numpy()
            legs["warm"].append(wall(lambda: db_u.batch_search("t", tq, k, filters=pats)))
            legs["batch_update_call"].append(wall(lambda: db_u.batch_update("t", [{"tenant": w} for w in who], vec)))
            b0 = built(db_u)
            legs["after_batch_update"].append(wall(lambda: db_u.batch_search("t", tq, k, filters=pats)))
            masks_built["after_batch_update"] += (built(db_u) - b0) if rep else 0

            def parent():
                for j, w in enumerate(who):
                    cnt = db_p.delete("t", {"tenant": w})
                    db_p.batch_add("t", np.repeat(vec[j:j + 1], cnt, axis=0), [{"id": "re", "tenant": w}] * cnt)

            legs["delete_and_batch_add_calls"].append(wall(parent))
            b0 = built(db_p)
            legs["after_delete_and_batch_add"].append(wall(lambda: db_p.batch_search("t", tq, k, filters=pats)))
            masks_built["after_delete_and_batch_add"] += (built(db_p) - b0) if rep else 0
        out["vecdb_batch_search"] = {
            "what": f"VecDB.batch_search, one query per tenant, all {T} tenant filters, right after batch_update of {U} tenants' rows vs right after "
                    f"delete + batch_add of the same rows on a twin table; 'warm' = the same search with nothing written before it",
            "tenants": T, "rows_per_tenant": n // T, "tenants_updated": U,
            **{name: summary(ts[1:]) for name, ts in legs.items()},
            "masks_built_by_the_searches": masks_built,
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
