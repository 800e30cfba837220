"""The outlier scores of csrc/outlier_plan.hpp restated in plain float64 numpy: N(p) = the first min(k, m - 1) allowed rows other than p in the
(distance, index) order, NaN greatest; kdist, reach = max(kdist(o), d(p, o)), lrd = 1 / (mean reach + 1e-10), lof = mean lrd(o) / lrd(p)."""
import numpy as np

RTOL = 1e-6  # both sides sum in f64 (the order cannot move a result by that much); the one rounding to f32 contributes 6e-8


def of_lists(nbr, nd, cnt):
    """(kdist f32, lrd f64, lof f64) [m] of lists nbr (items below m) / nd f32 [m][k] with cnt [m] counted slots each; NaN propagates"""
    nbr, nd, cnt = np.asarray(nbr, dtype=np.int64), np.asarray(nd, dtype=np.float32), np.asarray(cnt, dtype=np.int64)
    m, k = nd.shape
    used = np.arange(k)[None, :] < cnt[:, None]
    kdist = np.where(cnt > 0, nd[np.arange(m), np.maximum(cnt, 1) - 1], np.float32(np.nan)).astype(np.float32)
    with np.errstate(all="ignore"):
        reach = np.where(used, np.maximum(kdist[nbr], nd).astype(np.float64), 0.0)  # (np.maximum propagates NaN)
        lrd = 1.0 / (reach.sum(axis=1) / cnt + 1e-10)
        lof = np.where(used, lrd[nbr], 0.0).sum(axis=1) / cnt / lrd
    return kdist, lrd, lof


def graph_of_order(oi, od, k, allowed=None):
    """(rows, nbr as POSITIONS among rows, nd, cnt): oi / od [n][n] = every row's full order of all rows and its f32 distances; self out by id"""
    rows = np.arange(len(oi)) if allowed is None else np.flatnonzero(allowed)
    m, pos_of = len(rows), {int(r): p for p, r in enumerate(rows)}
    kk = min(k, m - 1)
    nbr, nd = np.zeros((m, k), dtype=np.int64), np.zeros((m, k), dtype=np.float32)
    for p, r in enumerate(rows.tolist()):
        keep = [j for j in range(len(oi[r])) if int(oi[r][j]) in pos_of and int(oi[r][j]) != r][:kk]
        nbr[p, :kk], nd[p, :kk] = [pos_of[int(oi[r][j])] for j in keep], od[r][keep]
    return rows, nbr, nd, np.full(m, kk, dtype=np.int64)


def order_of_matrix(D):
    """(oi, od): every row's order of all rows by (distance, index), NaN greatest, from a distance matrix in np.float32"""
    D = np.asarray(D, dtype=np.float32)
    oi = np.stack([np.lexsort((np.arange(len(D)), np.nan_to_num(d, nan=0.0, posinf=np.inf, neginf=-np.inf), np.isnan(d))) for d in D])
    return oi, np.take_along_axis(D, oi, axis=1)


def of_matrix(D, k, allowed=None):
    """(rows, kdist, lrd, lof) from a distance matrix in np.float32"""
    rows, nbr, nd, cnt = graph_of_order(*order_of_matrix(D), k, allowed)
    return (rows,) + of_lists(nbr, nd, cnt)


def close(got, want, rtol=RTOL):
    """got (f32) against want (f64): NaN where NaN, the same infinities, relative rtol elsewhere"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    assert (np.abs(got[fin] - want[fin]) <= rtol * np.abs(want[fin])).all(), float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin])))
