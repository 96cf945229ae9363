"""The neighbour-sparse t-SNE kernels (tsne_ops.hip) on the GPU against the restatement of the project's own definition
(tests/tsne_nbr_ref.py; include/tacorl_hip.h "neighbour-sparse t-SNE").  Lists and the CSR are compared bit for bit, conditionals
and forces are held to a-priori bounds, short trajectories to 4 x the deviation of the restatement run in fp32, the whole run to
the fixture's recorded fp64 results; and the embedding and the TSNEPlot callback run above the dense path's 8192 rows.  Every
case prints its figures in front of its assertions (tools/tsne_md.py collects them into profiles/tsne.md)."""
import functools
import types

import numpy as np
import pytest
import torch

from tests import tsne_nbr_ref as NR
from tests import tsne_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = np.int32


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(I32), np.ascontiguousarray(b).view(I32))


# ------------------------------------------------------------------------------------------ 1. neighbour lists
# (N, K, D, table).  The k-NN kernel stages the table in tiles of 128 rows (tacorl_tsne_nbr_knn_tile): 127 / 128 / 129.  K = 1 is
# run at N = 4, the smallest table the entry point takes (K + 1 = 2 is below it).
KNN_CASES = ([(max(K + 1, 4), K, 16, "loose") for K in (1, 63, 64, 65, 120, 192)] + [(257, K, 16, "loose") for K in (1, 63, 64, 65, 120, 192)]
             + [(1000, 120, 16, "loose"), (1000, 192, 32, "loose"), (1000, 1, 1, "loose"), (257, 65, 1, "loose"), (257, 64, 32, "loose"),
                (127, 63, 16, "loose"), (128, 64, 16, "loose"), (129, 65, 16, "loose"), (257, 65, 16, "wide"),
                (257, 63, 16, "ties"), (257, 1, 16, "ties"), (129, 65, 1, "ties"), (1000, 120, 32, "ties")])


@pytest.mark.parametrize("N,K,D,kind", KNN_CASES)
def test_neighbour_lists_bit_for_bit(N, K, D, kind):
    """Rows and distances against the fp32 NumPy restatement.  `ties`: groups of four identical rows - a row's duplicates lead
    its list at d = 0 in row order and the row itself is absent; `wide`: the rows are a column slice of a wider table."""
    from tacorl_amd import _lib, ops

    assert _lib.lib().tacorl_tsne_nbr_knn_tile() == 128
    X = NR.ties_table(N, D, N + K) if kind == "ties" else R.case_table(N, D, N + K)
    wide = np.full((N, D + (5 if kind == "wide" else 0)), 7.0, np.float32)
    wide[:, :D] = X
    rows, dist = ops.tsne_nbr_knn(_dev(wide)[:, :D], K)
    torch.cuda.synchronize()
    rows, dist = rows.cpu().numpy(), dist.cpu().numpy()
    want_r, want_d = NR.knn(X, K)
    assert want_d.dtype == np.float32
    assert (rows != np.arange(N)[:, None]).all()
    if kind == "ties" and K >= 3 and N % 4 == 0:
        grp = np.arange(N)[:, None] // 4 * 4 + np.arange(4)[None, :]
        assert np.array_equal(rows[:, :3], np.stack([g[g != i] for i, g in enumerate(grp)])) and not dist[:, :3].any()
    assert np.array_equal(rows, want_r) and _bits(dist, want_d)


# ------------------------------------------------------------------------------------------ 2. conditionals and CSR
def _table(kind, N, D):
    if kind == "fixture":
        return R.golden()["X"][:N]
    if kind == "hub":
        return NR.hub_table(N, D)
    return R.case_table(N, D, N, duplicates=kind == "dup")


@functools.lru_cache(maxsize=None)
def _aff(N, D=16, perp=None, kind="loose"):
    """The kernel's affinities of a case as host arrays (read-only, shared), CSR cut to row_ptr[N] entries."""
    from tacorl_amd import ops

    perp = R.perplexity_for(N) if perp is None else perp
    X = _table(kind, N, D)
    a = ops.tsne_nbr_affinities(_dev(X), perp)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in a.items() if k != "ws"}
    out["xn"] = ops.tsne_nbr_workspace_views(a["ws"], N)["xn"].cpu().numpy()
    nnz = int(out["row_ptr"][N])
    assert nnz <= 2 * N * NR.k_of(perp)
    out["col"], out["val"], out["X"], out["perp"] = out["col"][:nnz], out["val"][:nnz], X, perp
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


AFF_CASES = [(16, 16, None, "loose"), (121, 16, None, "loose"), (257, 16, None, "loose"), (1000, 16, None, "loose"), (257, 1, None, "loose"),
             (255, 32, None, "loose"), (257, 16, None, "dup"), (193, 16, 64.0, "fixture"), (300, 32, 10.0, "hub")]


@pytest.mark.parametrize("N,D,perp,kind", AFF_CASES)
def test_conditionals_and_csr(N, D, perp, kind):
    a = _aff(N, D, perp, kind)
    perp, K = a["perp"], NR.k_of(a["perp"])
    assert a["status"].tolist() == [0, 0]  # (a precondition of the inputs: these tables have no capped row)
    xn = a["xn"][:, :D]
    assert (np.abs(xn - R.normalise(a["X"])) <= R.normalise_allowance(a["X"])).all() and not a["xn"][:, D:].any()
    want_r, want_d = NR.knn(xn, K)  # the lists of the kernel's own normalised table
    assert np.array_equal(a["nbr_row"], want_r) and _bits(a["nbr_dist"], want_d)
    # p_{j|i} and H_i in fp64 at the kernel's betas, on the kernel's own lists
    d = NR.list_dists(xn.astype(np.float64), a["nbr_row"])
    b64 = a["beta"].astype(np.float64)
    use_h = use_c = 0.0
    for i in range(N):
        H, p = NR.row_entropy(d[i], b64[i])
        use_h = max(use_h, abs(H - np.log(perp)) / NR.entropy_allowance(d[i], b64[i], D))
        use_c = max(use_c, (np.abs(a["cond"][i] - p) / NR.cond_allowance(d[i], b64[i], D)).max())
    # the CSR of the kernel's own conditionals
    row_ptr, col, val = NR.csr(a["nbr_row"], a["cond"])
    total = a["val"].sum(dtype=np.float64)
    # each row's conditionals sum to 1 within the (K + 8) u of S and one division each; then one addition and one division
    sum_allow = R.sum_bound(K, 1.0) + 4 * R.U
    lens = np.diff(a["row_ptr"])
    print(f"tsne nbr affinities N={N} D={D} perp={perp:g} {kind}: allowance use H {use_h:.3f} p {use_c:.3f}; sum P - 1 {total - 1:.3g} "
          f"(bound {sum_allow:.3g}); row lengths {lens.min()} .. {lens.max()} (K = {K})")
    assert use_h <= 1 and use_c <= 1
    assert val.dtype == np.float32 and np.array_equal(a["row_ptr"], row_ptr) and np.array_equal(a["col"], col) and _bits(a["val"], val)
    assert abs(total - 1) <= sum_allow
    if kind == "hub":
        assert lens[0] == N - 1 > K and (a["nbr_row"][1:] == 0).any(1).all()


def test_hub_row_longer_than_the_in_lds_sort():
    """4200 rows around one centre: row 0 of the CSR has 4199 entries, past the 4096 the sort kernel takes into LDS - that row is
    sorted in place in global memory.  Lists and CSR bit for bit as above (the conditionals' allowances: the cases above)."""
    N, D = 4200, 32
    a = _aff(N, D, 10.0, "hub")
    assert a["status"].tolist() == [0, 0]
    want_r, want_d = NR.knn(a["xn"][:, :D], 30)
    assert np.array_equal(a["nbr_row"], want_r) and _bits(a["nbr_dist"], want_d)
    row_ptr, col, val = NR.csr(a["nbr_row"], a["cond"])
    assert row_ptr[1] == N - 1 > 4096
    assert np.array_equal(a["row_ptr"], row_ptr) and np.array_equal(a["col"], col) and _bits(a["val"], val)


# ------------------------------------------------------------------------------------------ 3. forces
def _synthetic_mid(N):
    """A mid-run state for a size neither fixture records: the rows of mid_1000 repeated, Y jittered (a spread map with spread
    gains; the forces depend on nothing else)."""
    src, idx = R.golden()["mid_1000"], np.arange(N) % 1000
    Y = src[0][idx] + (0.05 * np.random.RandomState(N).standard_normal((N, 2))).astype(np.float32)
    return Y.astype(np.float32), src[1][idx].copy(), src[2][idx].copy()


def _states(N):
    """The `init` and `mid` states of test_tsne_gpu._states where tsne_clusters.npz records the size; else the same init and the
    mid state of tsne_nbr_clusters.npz, or (511 .. 513, 8193: no fp64 run recorded) a synthetic one."""
    from tests.test_tsne_gpu import _states as dense_states

    if f"mid_{N}" in R.golden():
        return dense_states(N)
    Y0 = (1e-4 * np.random.RandomState(1000 + N).standard_normal((N, 2))).astype(np.float32)
    mid = NR.golden()[f"mid_{N}"] if f"mid_{N}" in NR.golden() else _synthetic_mid(N)
    return [("init", Y0, np.zeros_like(Y0), np.ones_like(Y0), 12.0, 0.5), ("mid", mid[0], mid[1], mid[2], 1.0, 0.8)]


def _gpu_steps(a, Y, u, g, ex, mom, n):
    """n kernel iterations from the state; (Y, u, gains, attr, rep, zrow of the LAST iteration) as host arrays."""
    from tacorl_amd import ops

    N = len(Y)
    csr = [_dev(a[k]) for k in ("row_ptr", "col", "val")]
    Yd, ud, gd = _dev(Y), _dev(u), _dev(g)
    ws = ops.tsne_nbr_workspace(N, DEV)
    for _ in range(n):
        ops.tsne_nbr_step(*csr, Yd, ud, gd, ex, mom, 200.0, ws)
    torch.cuda.synchronize()
    v = ops.tsne_nbr_workspace_views(ws, N)
    return [t.cpu().numpy() for t in (Yd, ud, gd, v["attr"], v["rep"], v["zrow"])]


def _bound_use(a, Y, got, rows):
    N = len(Y)
    attr, rep, zi, s_attr, s_rep, s_z, n = NR.forces_rows(a["row_ptr"], a["col"], a["val"], Y, rows)
    rows = np.asarray(rows)
    bounds = (R.sum_bound(n[:, None], s_attr), R.sum_bound(N, s_rep), R.sum_bound(N, s_z))
    return [(np.abs(g[rows] - r) / np.maximum(b, 1e-300)).max() for g, r, b in zip(got[3:6], (attr, rep, zi), bounds)], bounds


# 16 and 121 are K + 1 (perplexity 5 and 40).  The repulsion kernel's row block, its LDS tile of Y and (up to N = 8192) its
# segment are all 256 rows: 255 / 256 / 257, and 511 / 512 / 513 for the second segment's end.  8193 is the first size with
# segments of 512 (17 of them).
FORCE_NS = (16, 121, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 8193)
ROWS_8193 = np.concatenate([[0, 8192], 57 + 131 * np.arange(62)])  # the 64 rows compared at N = 8193


@pytest.mark.parametrize("N", FORCE_NS)
def test_forces_within_the_a_priori_bound(N):
    """(n + 8) u sum|term|: n = the row's stored entries for attr, N for rep and Z_i.  At N = 8193 the fp64 sums are taken for the
    64 fixed rows ROWS_8193 (the first, the last, 62 spread over the segments); two launches are compared on every row."""
    from tacorl_amd import _lib

    assert _lib.lib().tacorl_tsne_nbr_segment(N) == NR.segment(N) == (512 if N == 8193 else 256)
    a = _aff(N)
    rows = ROWS_8193 if N == 8193 else np.arange(N)
    assert len(rows) == 64 or N != 8193
    for name, Y, u, g, ex, mom in _states(N):
        got = _gpu_steps(a, Y, u, g, ex, mom, 1)
        use, _ = _bound_use(a, Y, got, rows)
        print(f"tsne nbr forces N={N} {name}: bound use attr {use[0]:.3f} rep {use[1]:.3f} Z_i {use[2]:.3f}")
        assert max(use) <= 1
        again = _gpu_steps(a, Y, u, g, ex, mom, 1)
        for x, y in zip(got, again):
            assert _bits(x, y)


# ------------------------------------------------------------------------------------------ 4. the full-neighbour limit
def test_full_neighbour_limit_meets_the_dense_path():
    """193 rows of the fixture table at perplexity 64: K = 192 = N - 1, every list is the whole table, and the definition is the
    dense one in real arithmetic.  attr, rep and Z_i of the two paths (each on its own P) differ by no more than the sum of
    their two summation bounds."""
    from tacorl_amd import ops

    N = 193
    a = _aff(N, 16, 64.0, "fixture")
    assert a["nbr_row"].shape == (N, N - 1) and (np.diff(a["row_ptr"]) == N - 1).all()
    P, _, status, ws = ops.tsne_affinities(_dev(a["X"]), 64.0)
    assert status.tolist() == [0, 0]
    P64 = P.cpu().numpy().astype(np.float64)
    for name, Y, u, g, ex, mom in _states(N):
        got = _gpu_steps(a, Y, u, g, ex, mom, 1)
        Yd, ud, gd = _dev(Y), _dev(u), _dev(g)
        ops.tsne_step(P, Yd, ud, gd, ex, mom, 200.0, ws)
        torch.cuda.synchronize()
        v = ops.tsne_workspace_views(ws, N)
        dense = [v[k].cpu().numpy() for k in ("attr", "rep", "zrow")]
        _, nb = _bound_use(a, Y, got, np.arange(N))
        s = R.forces(P64, Y.astype(np.float64))[3:]
        use = [(np.abs(x - y) / (b + R.sum_bound(N, t))).max() for x, y, b, t in zip(got[3:6], dense, nb, s)]
        print(f"tsne nbr full-neighbour limit N={N} {name}: |nbr - dense| / (sum of the two bounds): attr {use[0]:.3f} rep {use[1]:.3f} "
              f"Z_i {use[2]:.3f}")
        assert max(use) <= 1


# ------------------------------------------------------------------------------------------ 5. three steps
@pytest.mark.parametrize("N", (16, 63, 64, 65, 121, 257, 1000))
def test_three_steps_follow_the_fp64_restatement(N):
    """The rule of test_tsne_gpu.test_three_steps_follow_the_fp64_restatement: 4 x the deviation (Frobenius norm over Y, and over
    u) of the restatement run in fp32 with every sum in the stated order."""
    a = _aff(N)
    csr = (a["row_ptr"], a["col"], a["val"])
    for name, Y, u, g, ex, mom in _states(N):
        s64 = (Y.astype(np.float64), u.astype(np.float64), g.astype(np.float64))
        s32 = (Y, u, g)
        P64 = NR.dense(*csr, np.float64)
        for _ in range(3):
            s64 = R.step(P64, *s64, ex, mom, 200.0)
            s32 = NR.step_in_kernel_order(*csr, *s32, ex, mom, 200.0)
        assert s32[0].dtype == np.float32
        got = _gpu_steps(a, Y, u, g, ex, mom, 3)
        for k, what in ((0, "Y"), (1, "u")):
            dev32 = np.linalg.norm(s32[k].astype(np.float64) - s64[k])
            devk = np.linalg.norm(got[k].astype(np.float64) - s64[k])
            print(f"tsne nbr trajectory N={N} {name} {what}: kernel {devk:.3g}, fp32 restatement {dev32:.3g}, "
                  f"|{what}| {np.linalg.norm(s64[k]):.3g}")
            assert devk <= 4 * dev32


# ------------------------------------------------------------------------------------------ 6. KL
def test_kl_against_fp64():
    from tacorl_amd import ops

    N = 257
    a = _aff(N)
    Y = R.golden()[f"mid_{N}"][0]
    out = ops.tsne_nbr_kl(*[_dev(a[k]) for k in ("row_ptr", "col", "val")], _dev(Y), ops.tsne_nbr_workspace(N, DEV))
    got = float(out.item())
    P64, Y64 = NR.dense(a["row_ptr"], a["col"], a["val"], np.float64), Y.astype(np.float64)
    q = ((Y64[:, None] - Y64[None]) ** 2).sum(-1)
    w = 1 / (1 + q)
    np.fill_diagonal(w, 0)
    pos = P64 > 0
    mag = (P64[pos] * (np.abs(np.log(P64[pos])) + np.log1p(q[pos]))).sum() + (abs(np.log(w.sum())) + 1) * P64.sum()
    want = R.kl(P64, Y64)
    print(f"tsne nbr kl N={N}: kernel {got:.7g} fp64 {want:.7g}, bound use {abs(got - want) / R.sum_bound(N, mag):.3f}")
    assert abs(got - want) <= R.sum_bound(N, mag)


# ------------------------------------------------------------------------------------------ 7. the whole run
def test_whole_run_separates_the_fixture_clusters():
    from tacorl_amd.evaluation.tsne import tsne_embed_neighbours

    G, GN = R.golden(), NR.golden()
    Y, kl = tsne_embed_neighbours(_dev(G["X"]), perplexity=float(GN["perplexity"]), init=_dev(G["inits"][0].astype(np.float32)),
                                  return_kl=True)
    assert Y.shape == (240, 2) and Y.dtype == torch.float32 and Y.is_cuda
    acc = R.knn_accuracy(Y.cpu().numpy(), G["labels"])
    limit = GN["kl"].max() + (GN["kl"].max() - GN["kl"].min())
    print(f"tsne nbr whole run: KL {kl:.4f} (fp64 runs {GN['kl'].min():.4f} .. {GN['kl'].max():.4f}, limit {limit:.4f}), "
          f"5-NN accuracy {acc:.3f}")
    assert acc >= 0.98 and kl <= limit
    gen = torch.Generator(device=DEV).manual_seed(3)
    Y1 = tsne_embed_neighbours(_dev(G["X"]).view(6, 40, 16), perplexity=30.0, generator=gen)
    Y2 = tsne_embed_neighbours(_dev(G["X"]), perplexity=30.0, generator=torch.Generator(device=DEV).manual_seed(3))
    assert torch.equal(Y1, Y2) and R.knn_accuracy(Y1.cpu().numpy(), G["labels"]) >= 0.98


# ------------------------------------------------------------------------------------------ 8. above the old cap
def _clustered(N, D=16, seed=0):
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, 12, N)
    X = np.tanh(rs.uniform(-0.8, 0.8, (12, D))[lab] + 0.15 * rs.standard_normal((N, D))).astype(np.float32)
    return X, lab


def test_embedding_above_the_dense_cap():
    from tacorl_amd import ops
    from tacorl_amd.evaluation.tsne import tsne_embed_neighbours

    N = ops.TSNE_MAX_N + 8
    Y = tsne_embed_neighbours(_dev(_clustered(N)[0]), perplexity=40.0, n_iter=3)
    assert Y.shape == (N, 2) and Y.dtype == torch.float32 and bool(torch.isfinite(Y).all())


def _feed(plot, X, lab, batch=1000):
    mod = types.SimpleNamespace(global_step=5)
    for b, i in enumerate(range(0, len(X), batch)):
        plot.on_validation_batch_end(None, mod, {"sampled_plan_pp": _dev(X[i:i + batch])}, {"task_ids": torch.from_numpy(lab[i:i + batch])}, b)
    plot.on_validation_epoch_end(types.SimpleNamespace(logger=None), mod)
    return plot.last


@pytest.mark.parametrize("max_points", (None, 8500))
def test_tsneplot_maps_a_large_epoch(max_points):
    """9000 plans in one validation epoch: the map has them all, or - with max_points=8500 - the sorted subsample self.rng
    draws, labels alike."""
    from tacorl_amd.utils.callbacks.tsne_plot import TSNEPlot

    class Spy(TSNEPlot):  # keeps the rows handed to the embedding
        def _get_tsne(self, sampled_plans):
            self.embedded = sampled_plans.detach().cpu().numpy()
            return super()._get_tsne(sampled_plans)

    X, lab = _clustered(9000, seed=1)
    plot = Spy(40, 8, 0.1, 0.3, 5) if max_points is None else Spy(40, 8, 0.1, 0.3, 5, max_points=max_points)
    last = _feed(plot, X, lab)
    n = 9000 if max_points is None else max_points
    keep = np.arange(9000) if max_points is None else np.sort(np.random.RandomState(0).choice(9000, size=max_points, replace=False))
    assert _bits(plot.embedded, X[keep])  # the embedded rows are the rows the labels belong to, in their order
    assert last["x_tsne"].shape == (n, 2) and np.isfinite(last["x_tsne"]).all() and np.isfinite(last["kl"]) and last["step"] == 5
    if max_points is None:
        assert np.array_equal(last["labels"], lab)
        print(f"tsne nbr callback 9000 plans: KL {last['kl']:.4f}, 5-NN accuracy of every ninth point {R.knn_accuracy(last['x_tsne'][::9], lab[::9]):.3f}")
    else:
        assert np.array_equal(last["labels"], lab[keep])


# ------------------------------------------------------------------------------------------ 9. no change below the cap
def test_tsneplot_below_the_cap_is_tsne_embed():
    from tacorl_amd.evaluation.tsne import tsne_embed
    from tacorl_amd.utils.callbacks.tsne_plot import TSNEPlot

    G = R.golden()
    torch.manual_seed(11)
    last = _feed(TSNEPlot(30.0, 8, 1.0, 0.3, 5), G["X"], G["labels"].astype(np.int64), batch=100)
    torch.manual_seed(11)
    Y, kl = tsne_embed(_dev(G["X"]), perplexity=30.0, return_kl=True)
    assert _bits(last["x_tsne"], Y.cpu().numpy()) and last["kl"] == kl and last["x_tsne"].shape == (240, 2)
