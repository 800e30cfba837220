#!/usr/bin/env python3
"""What a row mask of a SET or RANGE predicate costs: vdb_mask_create_where_sets (k_mask_rows<MaskAll>) against the one-term equality mask of
vdb_mask_create_where -- which reads the same column bytes and is the yardstick -- and against the host loop over the metadata +
vdb_mask_create, the path such a filter took before.  Same process, same table, one run.

1M x 960 f32 rows (bench data, seed 1806) in a VecDB table; metadata per row: an id, `tenant` (1000 tenants x 1000 rows, row i belongs to
tenant i % 1000) and `year` (a string, 1990 .. 2024).  Timed, host clock around calls that end synchronised (every mask call does), median
of the repetitions:
  in_10          (a) GpuIndex.make_mask_where_sets for {"tenant": In(10 tenants)}: one term with a bitmap over the tenant codes
  ge_year        (b) the same for {"year": Ge(2010)}: evaluated over the year dictionary, one term
  eq_1           (c) GpuIndex.make_mask_where for {"tenant": "7"}: the one-term equality mask
  eq_1_as_set    the same term as {lo = hi = code} through make_mask_where_sets: same rows in, same rows out, only the kernel differs
  host_in_10 / host_ge_year   (d) the host loop (_Table.host_match) + GpuIndex.make_mask for (a) and (b)
  compile_*      LabelCodec.compile of (a) and (b): the host's share of the device path, O(distinct values)
and the kernels' own time for (a), (b), (c) from vdb_prof_get "mask_where_sets" / "mask_where" (separate profiled calls).
Every device-built mask is compared with the host path's mask of the same pattern (words and ids) before anything is timed.
Writes one JSON record (default profiles/mask_sets_1M.json)."""
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
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mask_sets_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import gist_like_gpu
    from lab_1806_vec_db_amd.labels import Ge, In
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
    t.metadata = [{"id": str(i), "tenant": str(i % T), "year": str(1990 + (i * 11) % 35)} for i in range(n)]

    def wall(fn, reps=args.reps):
        ts, out = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": reps}, out

    rec = {"what": "cost of a row mask of a set / range predicate: vdb_mask_create_where_sets vs the one-term equality mask of "
                   "vdb_mask_create_where (same column bytes) vs the host loop + vdb_mask_create; host clock around synchronised calls, same "
                   "process, same table, one run",
           "rows": n, "dim": dim, "tenants": T, "rows_per_tenant": n // T}
    p_in = {"tenant": In([str((37 * j + 5) % T) for j in range(10)])}
    p_ge = {"year": Ge(2010)}
    p_eq = {"tenant": "7"}

    # ---- (d) the host path, its two parts
    host = {}
    for name, p in (("host_in_10", p_in), ("host_ge_year", p_ge)):
        loop, allow = wall(lambda p=p: t.host_match(p), reps=3)
        mk_t, hm = wall(lambda allow=allow: ix.make_mask(allow))
        rec[name] = {"host_loop": loop, "make_mask": mk_t, "ms": loop["ms_median"] + mk_t["ms_median"], "allowed_rows": len(hm)}
        host[name] = hm

    t.create_columns([p_in, p_ge])
    assert t.codec.keys() == ["tenant", "year"] and ix.get_stat("label_columns") == 2

    # ---- the host's share of the device path
    rec["compile_in_10"], terms_in = wall(lambda: t.codec.compile(p_in), reps=4 * args.reps)
    rec["compile_ge_year"], terms_ge = wall(lambda: t.codec.compile(p_ge), reps=4 * args.reps)
    terms_eq = t.codec.terms(p_eq)
    rec["terms"] = {"in_10": repr(terms_in), "ge_year": repr(terms_ge), "bitmap_bytes_in_10": sum(tm.set_bits for tm in terms_in) // 8,
                    "bitmap_bytes_ge_year": sum(tm.set_bits for tm in terms_ge) // 8}

    # ---- identical to the host path's masks before anything is timed
    for terms, hm in ((terms_in, host["host_in_10"]), (terms_ge, host["host_ge_year"])):
        dm = ix.make_mask_where_sets(terms)
        assert all(np.array_equal(a, b) for a, b in zip(dm.rows(), hm.rows())) and len(dm) == len(hm)
        dm.close()
        hm.close()

    legs = (("in_10", lambda: ix.make_mask_where_sets(terms_in).close(), "mask_where_sets"),
            ("ge_year", lambda: ix.make_mask_where_sets(terms_ge).close(), "mask_where_sets"),
            ("eq_1_as_set", lambda: ix.make_mask_where_sets(terms_eq).close(), "mask_where_sets"),  # the same rows through the set kernel
            ("eq_1", lambda: ix.make_mask_where(terms_eq).close(), "mask_where"))
    for _, fn, _ in legs:  # warm-up
        fn()
    for name, fn, prof in legs:
        rec[name], _ = wall(fn, reps=8 * args.reps)
    preps = 8 * args.reps
    for name, fn, prof in legs:  # the kernels' own time: device events around the where + scan launches and around the ids launch
        ix.prof_enable(True)
        ix.prof_reset()
        for _ in range(preps):
            fn()
        p = ix.prof_get(prof)
        ix.prof_enable(False)
        rec[name]["kernels_ms"] = p["ms"] / preps
        rec[name]["kernel_launch_groups_per_call"] = p["launches"] / preps
    c = rec["eq_1"]
    rec["ratios"] = {
        "in_10_over_eq_1": rec["in_10"]["ms_median"] / c["ms_median"],
        "ge_year_over_eq_1": rec["ge_year"]["ms_median"] / c["ms_median"],
        "eq_1_as_set_over_eq_1": rec["eq_1_as_set"]["ms_median"] / c["ms_median"],
        "in_10_over_eq_1_kernels": rec["in_10"]["kernels_ms"] / c["kernels_ms"] if c["kernels_ms"] else None,
        "ge_year_over_eq_1_kernels": rec["ge_year"]["kernels_ms"] / c["kernels_ms"] if c["kernels_ms"] else None,
        "host_in_10_over_in_10": rec["host_in_10"]["ms"] / (rec["in_10"]["ms_median"] + rec["compile_in_10"]["ms_median"]),
        "host_ge_year_over_ge_year": rec["host_ge_year"]["ms"] / (rec["ge_year"]["ms_median"] + rec["compile_ge_year"]["ms_median"]),
        "note": "the ge_year mask allows about 43 % of the rows, the others 1 % and 0.1 %: a mask's allow-list (4 B per allowed row written "
                "by k_mask_ids) is part of every figure, so ge_year against eq_1 also compares different output sizes",
    }
    rec["mask_where_set_masks"] = ix.get_stat("mask_where_set_masks")
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    db.delete_table("t")


if __name__ == "__main__":
    main()
