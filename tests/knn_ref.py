"""Helpers of the neighbour-table tests: an fp64 brute-force k-NN oracle (written independently of the project's fp32 NumPy
restatement, tacorl_amd.data.neighbours.knn_l2_host), the NumPy statement of the margin filter, the test data and the golden."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nn_table.npz")


def knn_fp64(points, k):
    """(rows (N, min(k, N)), d64 (N, N)): all pairwise squared distances in fp64 as one vectorised sum over the columns, the
    neighbours ordered by (distance, row) with a lexicographic sort."""
    p = np.asarray(points, dtype=np.float64)
    n = len(p)
    d = np.empty((n, n))
    for b in range(0, n, 128):
        diff = p[b:b + 128, None, :] - p[None, :, :]
        d[b:b + 128] = np.einsum("qnd,qnd->qn", diff, diff)
    rows = np.empty((n, min(k, n)), dtype=np.int64)
    idx = np.arange(n)
    for q in range(n):
        rows[q] = np.lexsort((idx, d[q]))[: rows.shape[1]]
    return rows, d


def queries_needing_allowance(rows32, rows64, d64, D):
    """Compares ordered lists of an fp32 search with the fp64 oracle's.  Where they differ, the fp64 distances of the two
    differing entries must lie within relative 2 (D + 3) 2^-24 of each other - the two-sided bound of the D + 2 roundings of
    an fp32 sum of D non-negative terms (D multiplies / adds after D subtractions folded in), asserted here.  Returns how many
    queries needed that allowance."""
    tol = 2.0 * (D + 3) * 2.0 ** -24
    kk = rows64.shape[1]
    r32 = np.asarray(rows32)[:, :kk].astype(np.int64)
    assert (r32 >= 0).all()
    differ = r32 != rows64
    q, s = np.nonzero(differ)
    a, b = d64[q, r32[q, s]], d64[q, rows64[q, s]]
    bad = np.abs(a - b) > tol * np.maximum(a, b)
    assert not bad.any(), (q[bad][:5], s[bad][:5], a[bad][:5], b[bad][:5])
    return int(differ.any(axis=1).sum())


def margin_filter_np(nbr_row, q0, step_of_row, margin):
    """nn_steps (nq, k) int64 packed left / -1 after, count (nq) int32: the reference's rule, one neighbour at a time."""
    nbr_row = np.asarray(nbr_row)
    nq, k = nbr_row.shape
    out, cnt = np.full((nq, k), -1, dtype=np.int64), np.zeros(nq, dtype=np.int32)
    for i in range(nq):
        t = int(step_of_row[q0 + i])
        for r in nbr_row[i]:
            if r < 0:
                continue
            s = int(step_of_row[r])
            if not (s + margin > t > s - margin):
                out[i, cnt[i]] = s
                cnt[i] += 1
    return out, cnt


def normal_points(seed, n=1500, d=15):
    return np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)


def grid_points(seed=0, n=700, d=15):
    """Integer-grid points: every distance is an exact small integer, so nearly every query has a tie at the k-th place."""
    return np.random.RandomState(seed).randint(-2, 3, size=(n, d)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def golden():
    G = np.load(GOLDEN)
    nn = {int(k): v for k, v in json.loads(str(G["nn_json"]))["train"].items()}
    return {"robot_obs": G["robot_obs"], "ep": G["ep"], "num_nn": int(G["num_nn"]), "margin": int(G["margin"]), "nn": nn,
            "nn_json": str(G["nn_json"])}


def golden_points():
    g = golden()
    steps = np.concatenate([np.arange(s, e) for s, e in g["ep"]])
    return np.ascontiguousarray(g["robot_obs"][steps]), steps


@functools.lru_cache(maxsize=None)
def host_knn(kind, seed, k):
    """The fp32 restatement's (rows, distances) of a named data set, computed once per session."""
    from tacorl_amd.data.neighbours import knn_l2_host

    pts = {"normal": normal_points, "grid": grid_points}[kind](seed) if kind != "golden" else golden_points()[0]
    rows, dist = knn_l2_host(pts, k)
    rows.setflags(write=False), dist.setflags(write=False)
    return pts, rows, dist
