"""GpuIndex.silhouette at --rows x --dim (default 100 000 x 960) with --clusters labels (default 64 and 1024): wall time per call (median
of --reps after a warm-up), the three stages between events from prof_get (sil_prepare, sil_pairs, sil_finish), the f64 multiply-adds
the pair kernel issues (padded slots squared x dim, padding included) over its time, and what it is set against:

  baseline  the route a user had before: get_rows of a prefix of --baseline-rows rows and the full float64 distance matrix plus the
            cluster means in numpy on the host, timed on the prefix and EXTRAPOLATED by (rows / prefix)^2 to all rows (flagged in the
            record).

Synthetic data: Gaussian blobs, one per cluster, labels = the blob.  One run, medians, wall times around synchronised calls; not gated.
No rate of the f64 matrix pipe is known for these parts, so no share of a peak is derived.  Writes --out as JSON."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _host_route(x, labels):
    X = x.astype(np.float64)
    sq = (X * X).sum(1)
    D = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2 * X @ X.T, 0))
    values, own, size = np.unique(labels, return_inverse=True, return_counts=True)
    sums = np.stack([D[:, own == c].sum(1) for c in range(len(values))], 1)
    rows = np.arange(len(X))
    a = sums[rows, own] / np.maximum(size[own] - 1, 1)
    means = sums / size
    means[rows, own] = np.inf
    b = means.min(1)
    return np.where(size[own] > 1, (b - a) / np.maximum(np.maximum(a, b), 1e-300), 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--clusters", default="64,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-rows", type=int, default=8192)
    ap.add_argument("--out", default="profiles/flat_silhouette_100k.json")
    a = ap.parse_args()
    import torch

    import lab_1806_vec_db_amd as vdb

    res = {"rows": a.rows, "dim": a.dim, "reps": a.reps, "data": "synthetic Gaussian blobs, labels = the blob", "runs": []}
    for c in (int(v) for v in a.clusters.split(",")):
        rng = np.random.default_rng(c)
        centres = rng.standard_normal((c, a.dim), dtype=np.float32) * 2
        labels = rng.integers(0, c, a.rows).astype(np.uint32)
        ix = vdb.GpuIndex(a.dim, "l2sqr", device=0)
        for r0 in range(0, a.rows, 65536):
            nb = min(65536, a.rows - r0)
            ix.batch_add(centres[labels[r0:r0 + nb]] + rng.standard_normal((nb, a.dim), dtype=np.float32))
        ix.set_labels(0, labels)
        t_s = torch.zeros(a.rows, dtype=torch.float32, device="cuda")
        t_mean = torch.zeros(1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        call = lambda: ix.silhouette_device(0, t_s.data_ptr(), t_mean.data_ptr(), euclidean=True)
        ix.prof_enable(True)
        call()  # warm-up: allocations, code objects
        ix.prof_reset()
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            times.append(1e3 * (time.perf_counter() - t0))
        stages = {k: ix.prof_get(k)["ms"] / a.reps for k in ("sil_prepare", "sil_pairs", "sil_finish")}
        sizes = np.bincount(labels, minlength=c)
        plan = vdb.GpuIndex.silhouette_plan(a.rows, a.dim, sizes[sizes > 0])
        fma = float(plan[0]) ** 2 * a.dim
        nb = min(a.baseline_rows, a.rows)
        t0 = time.perf_counter()
        prefix = ix.get_rows(np.arange(nb, dtype=np.uint64))
        fetch_ms = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        host = _host_route(prefix, labels[:nb])
        host_ms = 1e3 * (time.perf_counter() - t0)
        res["runs"].append({"clusters": c, "call_ms": statistics.median(times), "stage_ms_between_events_per_call": stages,
                            "plan": dict(zip(("padded", "tiles", "slices", "mean_slots", "scratch_bytes"), plan[:5])),
                            "pair_kernel_f64_fma": fma, "pair_kernel_tflops_f64": 2e-9 * fma / max(stages["sil_pairs"], 1e-9),
                            "mean": float(t_mean.item()),
                            "host_route": {"rows_timed": nb, "EXTRAPOLATED_BY_ROWS_SQUARED": nb != a.rows, "get_rows_ms": fetch_ms * a.rows / nb,
                                           "numpy_float64_ms": host_ms * (a.rows / nb) ** 2, "prefix_mean": float(host.mean())}})
        ix.close()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
