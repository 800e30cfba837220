#!/usr/bin/env python3
"""What a row mask of a filter EXPRESSION costs: vdb_mask_create_where_any (k_mask_rows<MaskAny>, one pass over an OR of conjunctions) against
(a) the one-term equality mask of vdb_mask_create_where -- the yardstick of the mask line --, (b) the same normal form built clause by
clause with vdb_mask_create_where_sets_many and joined with vdb_mask_combine, and (c) the host loop over the metadata + vdb_mask_create,
the only path such a filter had before.  Same process, same table, one run.

1M x 960 f32 rows (bench data, seed 1806) in a VecDB table; metadata per row: an id, `tenant` (1000 tenants x 1000 rows, row i belongs to
tenant i % 1000), `year` (a string, 1990 .. 2024), `source` (3 values) and, on one row in 100, `shared`.  The expressions:
  or_shared    AnyOf({"tenant": "7"}, {"shared": "yes"})                                          2 clauses x 1 term
  and_or       AllOf({"tenant": In(10 tenants)}, AnyOf({"source": "web"}, {"year": Ge(2010)}))    2 clauses x 2 terms
  or_64        AnyOf of 64 patterns {"tenant": .., "year": ..}                                   64 clauses x 2 terms
Timed, host clock around calls that end synchronised (every mask call does), median of the repetitions (40 by default):
  <case>.any            GpuIndex.make_mask_where_any of the compiled clauses
  <case>.sets_combine   (b): ONE make_masks_where_sets call for the clauses, then combine_masks("or", ..) eight masks at a time
  <case>.host           (c): labels.matches_filter over the metadata + GpuIndex.make_mask
  <case>.compile        LabelCodec.compile_any: the host's share of the device path
  eq_1                  (a): GpuIndex.make_mask_where for {"tenant": "7"}
and the kernels' own time from vdb_prof_get "mask_where_any" / "mask_where_sets" + "mask_combine" / "mask_where" (separate profiled
calls), with the bytes the profile entry states (4 B x terms x rows over all clauses, bit words and allow-lists).
Every device-built mask is compared with the host path's mask of the same expression (words and ids) before anything is timed.
Writes one JSON record (default profiles/mask_any_1M.json)."""
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
    ap.add_argument("--tenants", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mask_any_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import gist_like_gpu
    from lab_1806_vec_db_amd.labels import AllOf, AnyOf, Ge, In, matches_filter
    from lab_1806_vec_db_amd.vecdb import VecDB

    dev = torch.device("cuda", 0)
    n, dim, T = args.rows, args.dim, args.tenants
    db = VecDB()
    db.create_table_if_not_exists("t", dim, "l2sqr")
    t = db._tables["t"]
    ix = t.index
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    ix.add_device(base.data_ptr(), n)  # (the rows go in from the device: a host copy of 3.84 GB is no part of what is measured)
    del base
    t.metadata = [{"id": str(i), "tenant": str(i % T), "year": str(1990 + (i * 11) % 35), "source": ("web", "mail", "scan")[(i // 7) % 3],
                   **({"shared": "yes"} if i % 100 == 0 else {})} for i in range(n)]

    def wall(fn, reps):
        ts, out = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": reps}, out

    reps = 8 * args.reps
    rec = {"what": "cost of a row mask of a filter expression: vdb_mask_create_where_any (one pass) vs the one-term equality mask vs the "
                   "clauses through vdb_mask_create_where_sets_many + vdb_mask_combine vs the host loop + vdb_mask_create; host clock around "
                   "synchronised calls, same process, same table, one run",
           "rows": n, "dim": dim, "tenants": T, "rows_per_tenant": n // T}
    exprs = {
        "or_shared": AnyOf({"tenant": "7"}, {"shared": "yes"}),
        "and_or": AllOf({"tenant": In([str((37 * j + 5) % T) for j in range(10)])}, AnyOf({"source": "web"}, {"year": Ge(2010)})),
        "or_64": AnyOf(*[{"tenant": t.metadata[r]["tenant"], "year": t.metadata[r]["year"]} for r in range(3, n, n // 64 + 4)][:64]),  # (the values of 64 rows: 64 tenants, no clause empty)
    }
    t.prepare(list(exprs.values()))
    assert sorted(t.codec.keys()) == ["shared", "source", "tenant", "year"] and ix.get_stat("label_columns") == 4

    def sets_combine(clauses):
        parts = ix.make_masks_where_sets(clauses)
        while len(parts) > 1:  # eight at a time, level by level
            nxt = [ix.combine_masks("or", parts[i:i + 8]) for i in range(0, len(parts), 8)]
            for mk in parts:
                mk.close()
            parts = nxt
        return parts[0]

    def profiled(fn, names):
        ix.prof_enable(True)
        ix.prof_reset()
        for _ in range(reps):
            fn()
        ps = [ix.prof_get(nm) for nm in names]
        ix.prof_enable(False)
        return {"kernels_ms": sum(p["ms"] for p in ps) / reps, "kernel_launch_groups_per_call": sum(p["launches"] for p in ps) / reps,
                "profile_bytes_per_call": sum(p["bytes"] for p in ps) / reps}

    terms_eq = t.codec.terms({"tenant": "7"})
    eq = lambda: ix.make_mask_where(terms_eq).close()  # noqa: E731
    eq()
    rec["eq_1"], _ = wall(eq, reps)
    rec["eq_1"].update(profiled(eq, ["mask_where"]))

    for name, e in exprs.items():
        r = rec[name] = {"expression": repr(e) if name != "or_64" else "AnyOf of 64 {tenant, year} patterns"}
        r["compile"], clauses = wall(lambda e=e: t.codec.compile_any(e), reps)
        r["clauses"], r["terms"] = len(clauses), sum(len(c) for c in clauses)
        assert name != "or_64" or r["clauses"] == 64
        loop, allow = wall(lambda e=e: np.fromiter((matches_filter(e, m) for m in t.metadata), dtype=np.bool_, count=n), 3)
        mk_t, hm = wall(lambda allow=allow: ix.make_mask(allow), args.reps)
        r["host"] = {"host_loop": loop, "make_mask": mk_t, "ms": loop["ms_median"] + mk_t["ms_median"]}
        r["allowed_rows"] = len(hm)
        # identical to the host path's mask before anything is timed, from every device path
        for dm in (ix.make_mask_where_any(clauses), sets_combine(clauses)):
            assert all(np.array_equal(a, b) for a, b in zip(dm.rows(), hm.rows())) and len(dm) == len(hm), name
            dm.close()
        hm.close()
        one = lambda clauses=clauses: ix.make_mask_where_any(clauses).close()  # noqa: E731
        one()
        r["any"], _ = wall(one, reps)
        r["any"].update(profiled(one, ["mask_where_any"]))
        two = lambda clauses=clauses: sets_combine(clauses).close()  # noqa: E731
        two()
        r["sets_combine"], _ = wall(two, reps)
        r["sets_combine"].update(profiled(two, ["mask_where_sets", "mask_combine"]))
        r["ratios"] = {
            "any_over_eq_1": r["any"]["ms_median"] / rec["eq_1"]["ms_median"],
            "any_over_eq_1_kernels": r["any"]["kernels_ms"] / rec["eq_1"]["kernels_ms"] if rec["eq_1"]["kernels_ms"] else None,
            "sets_combine_over_any": r["sets_combine"]["ms_median"] / r["any"]["ms_median"],
            "host_over_any": r["host"]["ms"] / (r["any"]["ms_median"] + r["compile"]["ms_median"]),
        }
    rec["counters"] = {s: ix.get_stat(s) for s in ("mask_where_any_masks", "mask_combine_masks", "mask_where_set_masks", "mask_where_masks")}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    db.delete_table("t")


if __name__ == "__main__":
    main()
