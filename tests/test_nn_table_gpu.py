"""The neighbour-table kernels on the GPU.  The search (`tacorl_knn_l2`) is compared BIT FOR BIT, rows and distances, with
the fp32 NumPy restatement (tacorl_amd.data.neighbours.knn_l2_host): the definition - direct-form fp32 distances, (distance,
row) order - makes that possible, so no tolerance is involved.  The margin filter is compared with its NumPy statement, and
the whole build with the file the unmodified reference class wrote (tests/golden/nn_table.npz)."""
import numpy as np
import pytest
import torch

from tests import knn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gpu(pts, k, **kw):
    from tacorl_amd import ops

    rows, dist = ops.knn_l2(pts if torch.is_tensor(pts) else torch.from_numpy(pts).to(DEV), k, **kw)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), dist.cpu().numpy()


def _same(rows, dist, rows_h, dist_h):
    assert rows.dtype == np.int32 and dist.dtype == np.float32 and rows.shape == rows_h.shape
    bad = np.nonzero((rows != rows_h).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], rows[bad[:2]], rows_h[bad[:2]])
    assert np.array_equal(dist.view(np.int32), dist_h.view(np.int32))  # the bits, +inf of the absent entries included


def _check(pts, k):
    from tacorl_amd.data.neighbours import knn_l2_host

    rows_h, dist_h = knn_l2_host(pts, k)
    rows, dist = _gpu(pts, k)
    _same(rows, dist, rows_h, dist_h)
    return rows, dist


def test_ties_go_to_the_lower_row():
    """Integer-grid points: every distance is an exact small integer, and for most queries (79 % of these) more rows sit at the
    k-th distance than the list has room for, so any deviation from the (distance, row) rule shows."""
    pts, rows_h, dist_h = R.host_knn("grid", 0, 32)
    cut = [np.sum(((pts - pts[q]) ** 2).sum(1) == dist_h[q, -1]) > np.sum(dist_h[q] == dist_h[q, -1]) for q in range(700)]
    assert np.mean(cut) > 0.7
    rows, dist = _gpu(pts, 32)
    _same(rows, dist, rows_h, dist_h)


def _edge_cases():
    from tacorl_amd import ops

    T, Q, Q64 = ops.KNN_TILE, ops.KNN_QUERY_BLOCK, ops.KNN_QUERY_BLOCK_K64
    cases = [(1, 15, 32), (5, 15, 32), (32, 15, 32), (64, 15, 64), (1, 1, 1), (2, 7, 2),
             (T - 1, 15, 32), (T, 15, 32), (T + 1, 15, 32), (2 * T + 3, 15, 32),
             (T - 1, 16, 64), (T, 32, 64), (T + 1, 1, 1), (2 * T + 3, 7, 2),
             (Q - 1, 7, 32), (Q, 16, 1), (Q + 1, 32, 2), (Q64 - 1, 15, 64), (Q64 + 1, 32, 64), (2 * Q + 5, 1, 64),
             (3 * T + 2, 32, 32), (3 * T + 1, 16, 2)]
    assert {c[1] for c in cases} == {1, 7, 15, 16, 32} and {c[2] for c in cases} == {1, 2, 32, 64}
    return cases


@pytest.mark.parametrize("N,D,k", _edge_cases())
def test_edges_of_the_blocking(N, D, k):
    """Table sizes around the LDS tile and the query block, every k / D family, tables smaller than k."""
    pts = np.random.RandomState(N * 100 + D + k).standard_normal((N, D)).astype(np.float32)
    if N > 4:
        pts[N - 1] = pts[1]          # a duplicate whose lower-row copy precedes the query itself
    rows, dist = _check(pts, k)
    if N < k:
        assert (rows[:, N:] == -1).all() and np.isposinf(dist[:, N:]).all() and (rows[:, :N] >= 0).all()
    if N > 4:
        assert rows[N - 1, 0] == 1 and dist[N - 1, 0] == 0 and (k == 1 or (rows[N - 1, 1] == N - 1 and dist[N - 1, 1] == 0))


def test_pitch_slices_and_determinism():
    """A column slice of a wider table (ld > D), a query slice (q0 > 0) against the full run, and two runs."""
    from tacorl_amd import ops
    from tacorl_amd.data.neighbours import knn_l2_host

    wide = torch.from_numpy(np.random.RandomState(3).standard_normal((700, 24)).astype(np.float32)).to(DEV)
    view = wide[:, 4:19]
    assert view.stride() == (24, 1)
    rows_h, dist_h = knn_l2_host(view.cpu().numpy(), 32)
    full = _gpu(view, 32)
    _same(*full, rows_h, dist_h)
    again = _gpu(view, 32)
    assert np.array_equal(full[0], again[0]) and np.array_equal(full[1].view(np.int32), again[1].view(np.int32))
    for q0, n in ((37, 200), (ops.KNN_QUERY_BLOCK + 1, 700 - ops.KNN_QUERY_BLOCK - 1), (699, 1)):
        part = _gpu(view, 32, q0=q0, n_queries=n)
        _same(*part, rows_h[q0:q0 + n], dist_h[q0:q0 + n])
    only_rows, none = ops.knn_l2(view, 32, want_dist=False)
    assert none is None and np.array_equal(only_rows.cpu().numpy(), rows_h)


@pytest.mark.parametrize("data", ["normal0", "normal1", "normal2", "golden"])
def test_continuous_data(data):
    """The standard-normal sets of the CPU test (N = 1500, D = 15, k = 32) and the smooth-trajectory golden points, whose
    near-duplicate consecutive frames are what the direct-form distance is for."""
    pts, rows_h, dist_h = R.host_knn("normal", int(data[-1]), 32) if data != "golden" else R.host_knn("golden", 0, 32)
    rows, dist = _gpu(pts, 32)
    _same(rows, dist, rows_h, dist_h)


def test_long_table_in_query_slices():
    """157 tiles of a random-walk table (consecutive rows near-duplicates: approaching its own neighbourhood a query inserts
    row after row): two query slices against the restatement of the same rows."""
    from tacorl_amd.data.neighbours import knn_l2_host

    walk = np.cumsum(0.01 * np.random.RandomState(5).standard_normal((20001, 15)), axis=0).astype(np.float32)
    pts = torch.from_numpy(walk).to(DEV)
    for q0, n in ((0, 100), (19871, 130)):
        _same(*_gpu(pts, 32, q0=q0, n_queries=n), *knn_l2_host(walk, 32, q0=q0, n_queries=n))


def test_margin_filter_against_its_numpy_statement():
    from tacorl_amd import ops

    steps = np.concatenate([np.arange(0, 50), np.arange(60, 130), np.arange(200, 260)]).astype(np.int64)  # gaps between episodes
    n, k, margin = len(steps), 8, 16
    row_of = {int(s): r for r, s in enumerate(steps)}
    rs = np.random.RandomState(0)
    nbr = rs.randint(0, n, size=(n, k)).astype(np.int32)
    nbr[rs.random_sample((n, k)) < 0.2] = -1                     # absent entries anywhere in a list
    nbr[5] = -1                                                  # ... and a list of nothing else
    # query step 100 (row 90): |dt| = margin - 1, margin, margin + 1 on both sides, itself and an absent entry
    q = row_of[100]
    nbr[q] = [row_of[100 - 15], row_of[100 + 15], row_of[100 - 16], -1, row_of[100 + 16], row_of[100 - 17], row_of[100 + 17], q]
    # ... and across an episode gap: steps 49 and 60 are 11 apart although they are neighbours in row order
    nbr[row_of[49]] = [row_of[60], row_of[65], row_of[64], row_of[33], row_of[34], row_of[49], -1, row_of[66]]
    d_nbr, d_steps = torch.from_numpy(nbr).to(DEV), torch.from_numpy(steps).to(DEV)
    for m in (16, 0, 1, 10 ** 12):
        out = torch.full((n, k), 7777, dtype=torch.int64, device=DEV)
        cnt = torch.full((n,), 7777, dtype=torch.int32, device=DEV)
        ops.nn_margin_filter(d_nbr, d_steps, m, nn_steps=out, count=cnt)
        exp, exp_cnt = R.margin_filter_np(nbr, 0, steps, m)
        assert np.array_equal(out.cpu().numpy(), exp) and np.array_equal(cnt.cpu().numpy(), exp_cnt)  # every element written
        if m == 0:
            assert np.array_equal(exp_cnt, (nbr >= 0).sum(1))   # margin 0 drops nothing but the absent entries
        if m == 10 ** 12:
            assert exp_cnt.sum() == 0 and (exp == -1).all()     # a huge margin drops everything
    exp, exp_cnt = R.margin_filter_np(nbr, 0, steps, margin)
    assert exp[q].tolist() == [84, 116, 83, 117, -1, -1, -1, -1] and exp_cnt[q] == 4
    assert exp[row_of[49]].tolist() == [65, 33, 66, -1, -1, -1, -1, -1]
    # a query slice: rows [q0, q0 + nq) of the same table
    q0, nq = 41, 100
    out, cnt = ops.nn_margin_filter(d_nbr[q0:q0 + nq].contiguous(), d_steps, margin, q0=q0)
    assert np.array_equal(out.cpu().numpy(), exp[q0:q0 + nq]) and np.array_equal(cnt.cpu().numpy(), exp_cnt[q0:q0 + nq])


def test_build_equals_the_reference_file_and_feeds_the_transition_replay():
    from tacorl_amd.data.neighbours import build_nn_steps_from_step
    from tacorl_amd.data.replay import HbmTransitionReplay, TransitionIndex

    g = R.golden()
    tab = build_nn_steps_from_step(g["robot_obs"], g["ep"], g["num_nn"], g["margin"], device=DEV)
    assert tab.to_dict() == g["nn"]                                # key for key, list for list, in order
    assert tab.ptr.is_cuda and tab.ptr.dtype == tab.val.dtype == torch.int64 and tab.ptr.numel() == 301 and tab.n_frames == 300
    # in slices, and from a tensor already on the device: the same table
    for obs, qb in ((g["robot_obs"], 100), (torch.from_numpy(g["robot_obs"]).to(DEV), 1), (torch.from_numpy(g["robot_obs"]).double(), None)):
        t2 = build_nn_steps_from_step(obs, g["ep"], g["num_nn"], g["margin"], device=DEV, query_block=qb)
        assert torch.equal(t2.ptr, tab.ptr) and torch.equal(t2.val, tab.val) and torch.equal(t2.steps, tab.steps)
    # strategy-1 goals out of a replay built from the table are those of one built from the dict
    probs = {"geometric": 0.5, "similar_robot_obs": 0.5}
    ia = TransitionIndex(g["ep"], n_frames=300, goal_strategy_prob=probs, nn_steps_from_step=tab)
    ib = TransitionIndex(g["ep"], n_frames=300, goal_strategy_prob=probs, nn_steps_from_step=tab.to_dict())
    acts = np.random.RandomState(0).uniform(-1, 1, size=(300, 7)).astype(np.float32)
    ra = HbmTransitionReplay({}, acts, ia, device=DEV, batch_size=8)
    rb = HbmTransitionReplay({}, acts, ib, device=DEV, batch_size=8)
    assert ra.tables["nn_val"].data_ptr() == tab.val.data_ptr() and ra.tables["nn_ptr"].data_ptr() == tab.ptr.data_ptr()
    assert torch.equal(ra.tables["nn_ptr"], rb.tables["nn_ptr"]) and torch.equal(ra.tables["nn_val"], rb.tables["nn_val"])
    d = ia.draw(2000, np.random.default_rng(7))
    s = ib.sample(None, d)
    ba, bb = ra.batch(d, fused=True), rb.batch(d, fused=True)
    ids_a, ids_b = ba["replay"]["ids"].cpu().numpy(), bb["replay"]["ids"].cpu().numpy()
    assert np.array_equal(ids_a, ids_b) and np.array_equal(ids_a, np.stack([s["step"], s["next"], s["goal"]]))
    sim = (d["strategy"] == 1)
    assert (sim & np.isin(ids_a[2], tab.val.cpu().numpy())).sum() > 100 and sim.sum() > 500  # neighbour goals were drawn
    ra.check(), rb.check()
