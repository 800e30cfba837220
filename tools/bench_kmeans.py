"""One Lloyd iteration of GpuIndex.kmeans at --rows x --dim (default 1M x 960) with c in --clusters (default 64, 1024): wall time per
iteration and the assign / resolve / update times from prof_get, the share of rows the matrix pass left to the exact fold, and a baseline.

The baseline is the exact-scan route the IVF trainer's assignment step stands for: the centroids as a flat_mode = 1 index, the rows as its
queries in chunks of 8192, k = 1 (one strict fold per pair, no matrix instruction), timed over --baseline-rows rows and EXTRAPOLATED to all
rows, plus the update on the host (a stable argsort by cluster and np.add.reduceat in float32, timed on the same rows and extrapolated).
The trainer's own assign_nearest is private to the library; this is the same arithmetic through the public search.

Synthetic data: `--blobs` Gaussian blobs (unit-cube centres, sigma 0.1 per coordinate).  One run, wall times.  Writes --out as JSON."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--clusters", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--blobs", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--baseline-rows", type=int, default=65536)
    ap.add_argument("--out", default="profiles/flat_kmeans_1M.json")
    a = ap.parse_args()
    import torch

    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(1)
    centres = rng.random((a.blobs, a.dim), dtype=np.float32)
    ix = vdb.GpuIndex(a.dim, "l2sqr", device=0)
    sample = None
    for r0 in range(0, a.rows, 65536):
        nb = min(65536, a.rows - r0)
        x = centres[rng.integers(0, a.blobs, nb)] + rng.standard_normal((nb, a.dim), dtype=np.float32) * np.float32(0.1)
        ix.batch_add(x)
        if sample is None:
            sample = x[: a.baseline_rows].copy()
    ix.prof_enable(True)
    res = {"rows": a.rows, "dim": a.dim, "blobs": a.blobs, "data": "synthetic Gaussian blobs, sigma 0.1", "cases": []}
    for c in a.clusters:
        init = ix.get_rows(np.arange(c, dtype=np.uint64) * (a.rows // c))
        ix.kmeans(c, max_iter=1, init=init)  # warm-up: allocations, code objects
        ix.prof_reset()
        s0 = {k: ix.get_stat(k) for k in ("kmeans_rows_assigned", "kmeans_unsure_rows")}
        t0 = time.perf_counter()
        _, assign, _, iters, _ = ix.kmeans(c, max_iter=a.iters, tol=0.0, init=init)
        wall = time.perf_counter() - t0
        steps = iters + 1  # assignment steps
        prof = {k: ix.prof_get(k)["ms"] / steps for k in ("kmeans_assign", "kmeans_resolve", "kmeans_update")}
        assigned = ix.get_stat("kmeans_rows_assigned") - s0["kmeans_rows_assigned"]
        unsure = ix.get_stat("kmeans_unsure_rows") - s0["kmeans_unsure_rows"]
        # the baseline on a sample of the rows
        cx = vdb.GpuIndex(a.dim, "l2sqr", device=0)
        cx.batch_add(init)
        cx.set_flat_mode(1)
        q = torch.from_numpy(sample).cuda()
        o_i = torch.zeros(8192, dtype=torch.int64, device="cuda")
        o_d = torch.zeros(8192, dtype=torch.float32, device="cuda")
        o_c = torch.zeros(8192, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for r0 in range(0, len(sample), 8192):
            nb = min(8192, len(sample) - r0)
            cx.flat_knn_device(q[r0:].data_ptr(), nb, 1, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr())
        base_assign = (time.perf_counter() - t0) * a.rows / len(sample)
        t0 = time.perf_counter()
        sa = assign[: len(sample)]
        order = np.argsort(sa, kind="stable")
        starts = np.flatnonzero(np.r_[True, np.diff(sa[order]) != 0])
        np.add.reduceat(sample[order], starts, axis=0)
        base_update = (time.perf_counter() - t0) * a.rows / len(sample)
        cx.close()
        case = {"clusters": c, "assignment_steps": steps, "wall_ms_per_step": 1e3 * wall / steps, "prof_ms_per_step": prof,
                "unsure_share": unsure / max(assigned, 1), "baseline_rows_timed": len(sample),
                "baseline_assign_ms_extrapolated": 1e3 * base_assign, "baseline_host_update_ms_extrapolated": 1e3 * base_update}
        print(json.dumps(case), flush=True)
        res["cases"].append(case)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    ix.close()


if __name__ == "__main__":
    main()
