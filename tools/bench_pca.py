"""GpuIndex.covariance and GpuIndex.project at --rows x --dim (default 1M x 960): wall time per call (median of --reps after a warm-up),
the three stages of the covariance between events from prof_get (pca_mean, pca_cov, pca_cov_reduce), and what they are set against:

  floor     vdb_stream_probe_rows over the same number of bytes at the table's row size: the time of ONE read of the table.  The covariance
            reads it once for the mean and once per block column for the blocks, so this is a floor, not a target.
  baseline  the route a user had before: get_rows of a prefix of --baseline-rows rows and np.cov in float64 on the host, timed on the
            prefix and EXTRAPOLATED linearly to all rows (flagged in the record); for project, the float64 matrix product on the host.

Synthetic data: a low-rank corpus (--rank latent dimensions through a random map, plus noise and an offset).  One run, medians, wall
times around synchronised calls; not gated.  No rate of the f64 matrix pipe is known for these parts, so no share of a peak is derived.
Writes --out as JSON."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fn, reps):
    fn()  # warm-up: allocations, code objects
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--components", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-rows", type=int, default=65536)
    ap.add_argument("--out", default="profiles/flat_pca_1M.json")
    a = ap.parse_args()
    import torch

    import lab_1806_vec_db_amd as vdb
    from lab_1806_vec_db_amd.index import stream_probe_rows

    rng = np.random.default_rng(1)
    lift = rng.standard_normal((a.rank, a.dim), dtype=np.float32)
    offset = rng.standard_normal(a.dim, dtype=np.float32) * 2
    ix = vdb.GpuIndex(a.dim, "l2sqr", device=0)
    for r0 in range(0, a.rows, 65536):
        nb = min(65536, a.rows - r0)
        ix.batch_add(rng.standard_normal((nb, a.rank), dtype=np.float32) @ lift + rng.standard_normal((nb, a.dim), dtype=np.float32) * np.float32(0.05) + offset)
    t_mean = torch.zeros(a.dim, dtype=torch.float64, device="cuda")
    t_cov = torch.zeros((a.dim, a.dim), dtype=torch.float64, device="cuda")
    t_out = torch.zeros((a.rows, a.components), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ix.prof_enable(True)
    ix.covariance_device(t_mean.data_ptr(), t_cov.data_ptr())
    ix.prof_reset()
    cov_ms = _median_ms(lambda: ix.covariance_device(t_mean.data_ptr(), t_cov.data_ptr()), a.reps)
    stages = {k: ix.prof_get(k)["ms"] / max(ix.prof_get(k)["launches"], 1) for k in ("pca_mean", "pca_cov", "pca_cov_reduce")}
    w, v = np.linalg.eigh(t_cov.cpu().numpy())
    t_w = torch.from_numpy(np.ascontiguousarray(v[:, ::-1].T[: a.components], dtype=np.float32)).cuda()
    ix.prof_reset()
    proj_ms = _median_ms(lambda: ix.project_device(t_w.data_ptr(), a.components, t_out.data_ptr(), t_mean.data_ptr()), a.reps)
    proj_kernel = ix.prof_get("pca_project")["ms"] / max(ix.prof_get("pca_project")["launches"], 1)
    table_bytes = a.rows * a.dim * 4
    gbps = stream_probe_rows(0, table_bytes, 5, a.dim * 4)
    # the host route on a prefix
    nb = min(a.baseline_rows, a.rows)
    t0 = time.perf_counter()
    prefix = ix.get_rows(np.arange(nb, dtype=np.uint64))
    fetch_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    p64 = prefix.astype(np.float64)
    np.cov(p64, rowvar=False)
    host_cov_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    (p64 - p64.mean(0)) @ v[:, ::-1][:, : a.components]
    host_proj_ms = 1e3 * (time.perf_counter() - t0)
    scale = a.rows / nb
    res = {"rows": a.rows, "dim": a.dim, "components": a.components, "reps": a.reps, "data": f"synthetic rank {a.rank} + noise 0.05 + offset",
           "plan": dict(zip(("dim_pad", "blocks", "segments", "seg_rows", "scratch_bytes"), vdb.GpuIndex.pca_plan(a.rows, a.dim))),
           "covariance_ms": cov_ms, "covariance_stage_ms_between_events": stages, "explained_by_first_rank": float(w[::-1][: a.rank].sum() / w.sum()),
           "project_ms": proj_ms, "project_kernel_ms_between_events": proj_kernel,
           "one_read_floor": {"probe_gbps": gbps, "table_bytes": table_bytes, "ms": 1e3 * table_bytes / (gbps * 1e9)},
           "host_route": {"rows_timed": nb, "EXTRAPOLATED": scale != 1.0, "get_rows_ms": fetch_ms * scale, "np_cov_float64_ms": host_cov_ms * scale,
                          "np_project_float64_ms": host_proj_ms * scale}}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    ix.close()


if __name__ == "__main__":
    main()
