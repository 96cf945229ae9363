"""The fp64 restatement of the neighbour-sparse t-SNE (tests/tsne_nbr_ref.py) and the allowances its GPU tests use, checked
without a GPU: the fixture regenerates, the definition has the properties it must have (the full-neighbour limit is the dense
definition), the a-priori bounds hold for an fp32 evaluation in the stated order and are discriminating, and the entry points
refuse bad arguments before they touch a device."""
import ctypes as C

import numpy as np
import pytest

from tests import tsne_nbr_ref as NR
from tests import tsne_ref as R


def test_fixture_is_the_restatements():
    G, D = NR.golden(), R.golden()
    assert float(G["perplexity"]) == float(D["perplexity"]) == 30.0 and G["kl"].shape == G["kl0"].shape == G["acc"].shape == (8,)
    a = NR.affinities(D["X"], 30.0)
    assert a[-1] == 0
    P = NR.dense(*a[:3])
    assert abs(R.kl(P, D["inits"][0]) - G["kl0"][0]) < 1e-9
    assert (G["acc"] == 1.0).all() and G["kl"].max() - G["kl"].min() < 0.02 and G["kl"].min() > 0.05
    for N in (121, 256):
        mid = G[f"mid_{N}"]
        assert mid.shape == (3, N, 2) and mid.dtype == np.float32 and mid[2].min() >= 0.01 and mid[2].max() > 2


def test_definition_properties():
    X = R.case_table(257, 16, 257)
    row_ptr, col, val, rows, dists, cond, betas, capped = NR.affinities(X, 40.0)
    N, K = 257, 120
    assert capped == 0 and rows.shape == (N, K) and NR.k_of(40.0) == K and NR.k_of(1.0) == 3 and NR.k_of(64.0) == 192
    assert (rows != np.arange(N)[:, None]).all() and (np.diff(dists, axis=1) >= 0).all()
    H = np.array([NR.row_entropy(dists[i], betas[i])[0] for i in range(N)])
    assert np.abs(H - np.log(40.0)).max() < 1e-5 and np.abs(cond.sum(1) - 1).max() < 1e-12
    P = NR.dense(row_ptr, col, val)
    assert np.array_equal(P, P.T) and not P.diagonal().any() and abs(P.sum() - 1) < 1e-12
    lens = np.diff(row_ptr)
    assert lens.min() >= K and row_ptr[N] <= 2 * N * K and all((np.diff(col[row_ptr[i]:row_ptr[i + 1]]) > 0).all() for i in range(N))
    assert NR.segment(8192) == 256 and NR.segment(8193) == 512 and NR.segment(131072) == 4096 and NR.segment(4) == 256


def test_hub_and_ties_tables():
    X = NR.hub_table()
    row_ptr, col, val, rows, *_ = NR.affinities(X, 10.0)
    assert (rows[1:] == 0).any(1).all() and row_ptr[1] - row_ptr[0] == len(X) - 1 > NR.k_of(10.0)  # the centre is in every list
    T = NR.ties_table(41, 3, 1)
    rows, d = NR.knn(R.normalise(T, np.float32), 5)
    assert (d[:40, :3] == 0).all() and rows[5, :3].tolist() == [4, 6, 7] and rows[4, :3].tolist() == [5, 6, 7] and (d[40] > 0).all()


def test_lists_are_total_for_non_finite_tables():
    """The rule the kernels rely on for their addressing: a NaN distance counts as +inf, so every list holds K valid other
    rows.  One NaN reaches every row of the normalised table (through its column's mean): every distance is NaN, and each
    list is the K lowest other rows at +inf.  NaN in some rows only: those rows go last in the others' lists."""
    X = R.case_table(41, 4, 41)
    X[7, 2] = np.nan
    with np.errstate(invalid="ignore"):
        xn = R.normalise(X, np.float32)
    assert np.isnan(xn[:, 2]).all()
    rows, d = NR.knn(xn, 5)
    assert np.isinf(d).all() and all(rows[i].tolist() == [j for j in range(7) if j != i][:5] for i in range(41))
    Z = R.case_table(41, 4, 41)
    Z[[3, 9]] = np.nan
    rows, d = NR.knn(Z, 40)
    assert (rows >= 0).all() and (rows < 41).all() and (rows != np.arange(41)[:, None]).all()
    assert sorted(rows[0, -2:].tolist()) == [3, 9] and np.isinf(d[0, -2:]).all() and np.isfinite(d[0, :-2]).all()
    assert rows[3].tolist() == [j for j in range(41) if j != 3] and np.isinf(d[3]).all()


def test_full_neighbour_limit_is_the_dense_definition():
    """K = N - 1: every list is the whole table and P is the dense definition's matrix (fp64: to rounding)."""
    X = R.golden()["X"][:193]
    a = NR.affinities(X, 64.0)
    assert a[3].shape == (193, 192)
    Pd = R.affinities(X, 64.0)[0]
    assert np.abs(NR.dense(*a[:3]) - Pd).max() <= 1e-12 * Pd.max()


@pytest.mark.parametrize("N", (16, 257, 1000))
def test_the_ordered_statement_is_the_same_function(N):
    G = R.golden()
    row_ptr, col, val = NR.affinities(R.case_table(N, 16, N), R.perplexity_for(N))[:3]
    s = tuple(a.astype(np.float64) for a in G[f"mid_{N}"])
    a, b = R.step(NR.dense(row_ptr, col, val), *s, 1.0, 0.8, 200.0), NR.step_in_kernel_order(row_ptr, col, val, *s, 1.0, 0.8, 200.0)
    assert np.array_equal(a[2], b[2])
    for x, y in zip(a[:2], b[:2]):
        assert np.abs(x - y).max() <= 1e-10 * np.abs(x).max()


def _fp32_sums(row_ptr, col, val32, Y):
    """attr, rep, Z_i of an fp32 machine in the stated order."""
    N = len(Y)
    dx, dy = Y[:, None, 0] - Y[None, :, 0], Y[:, None, 1] - Y[None, :, 1]
    w = np.float32(1) / (np.float32(1) + (dx * dx + dy * dy))
    np.fill_diagonal(w, 0)
    ri, ci = np.repeat(np.arange(N), np.diff(row_ptr)), col
    pw = val32 * w[ri, ci]
    assert pw.dtype == np.float32
    return (np.stack([NR._wave_rows_csr(row_ptr, pw * dx[ri, ci]), NR._wave_rows_csr(row_ptr, pw * dy[ri, ci])], 1),
            np.stack([NR._segment_rows(w * w * dx), NR._segment_rows(w * w * dy)], 1), NR._segment_rows(w))


@pytest.mark.parametrize("N", (16, 63, 257, 1000))
def test_force_bound_holds_for_fp32_and_is_discriminating(N):
    """(n + 8) u sum|term| per row and component (n = the row's stored entries for attr, N for rep and Z_i): the fp32 evaluation
    in the stated order stays inside it; a row that reports its neighbour row's sums (a one-row fault) leaves it by at least
    10 x in one of its five numbers, for every row, at both states."""
    G = R.golden()
    row_ptr, col, val = NR.affinities(R.case_table(N, 16, N), R.perplexity_for(N))[:3]
    val32 = val.astype(np.float32)
    Y0 = (1e-4 * np.random.RandomState(1000 + N).standard_normal((N, 2))).astype(np.float32)
    for name, Y in (("init", Y0), ("mid", G[f"mid_{N}"][0])):
        attr, rep, zi, s_attr, s_rep, s_z, n = NR.forces_rows(row_ptr, col, val32, Y, range(N))
        bounds = (R.sum_bound(n[:, None], s_attr), R.sum_bound(N, s_rep), R.sum_bound(N, s_z))
        got = _fp32_sums(row_ptr, col, val32, Y)
        use = max((np.abs(g - r) / b).max() for g, r, b in zip(got, (attr, rep, zi), bounds))
        nxt = np.roll(np.arange(N), -1)
        fault = np.max([(np.abs(r[nxt] - r) / b).reshape(N, -1).max(1) for r, b in zip((attr, rep, zi), bounds)], axis=0)
        print(f"nbr N={N} {name}: fp32 in the stated order uses {use:.3f} of the bound; a one-row fault is >= {fault.min():.3g} x the bound")
        assert use <= 1 and fault.min() >= 10


@pytest.mark.parametrize("N,D", [(16, 16), (63, 1), (257, 16), (257, 32), (1000, 16)])
def test_affinity_allowances_hold_for_fp32_and_are_discriminating(N, D):
    """The fp32 run of the restatement (its own lists and betas) is inside the allowances for H_i, p_{j|i} and the stored P_e,
    evaluated in fp64 at those betas on the fp32 lists' pairs of the fp32-normalised table; a stored entry without its larger
    half (a one-entry fault) is off by at least 10 x its allowance."""
    X, perp = R.case_table(N, D, N), R.perplexity_for(N)
    K = NR.k_of(perp)
    xn32 = R.normalise(X, np.float32)
    rows, d32 = NR.knn(xn32, K)
    assert d32.dtype == np.float32
    c32, b32, capped = NR.conditionals(d32, perp)
    assert capped == 0 and c32.dtype == np.float32 and b32.dtype == np.float32
    d = NR.list_dists(xn32.astype(np.float64), rows)
    b = b32.astype(np.float64)
    c64 = NR.cond_rows(d, b)
    for i in range(N):
        assert abs(NR.row_entropy(d[i], b[i])[0] - np.log(perp)) <= NR.entropy_allowance(d[i], b[i], D)
        assert (np.abs(c32[i] - c64[i]) <= NR.cond_allowance(d[i], b[i], D)).all()
    rp32, col32, v32 = NR.csr(rows, c32)
    rp, col, v = NR.csr(rows, c64)
    assert v32.dtype == np.float32 and np.array_equal(rp32, rp) and np.array_equal(col32, col)
    allow = NR.val_allowance(rows, d, b, D)
    assert (np.abs(v32 - v) <= allow).all()
    C64, _ = NR.scatter(rows, c64)
    ri = np.repeat(np.arange(N), np.diff(rp))
    big = np.maximum(C64[ri, col], C64[col, ri]) / (2 * N)
    top = np.array([e0 + big[e0:e1].argmax() for e0, e1 in zip(rp[:-1], rp[1:])])  # each row's largest half
    ratio = (big / allow)[top]
    print(f"nbr N={N} D={D}: one-entry fault / allowance: min {ratio.min():.1f}; fp32 uses {(np.abs(v32 - v) / allow).max():.3f}")
    assert ratio.min() >= 10


def test_entry_points_refuse_before_any_launch():
    """No GPU here: every call below must come back from its argument checks."""
    from tacorl_amd import _lib, ops

    L = _lib.lib()
    cap, kmax = L.tacorl_tsne_nbr_max_n(), L.tacorl_tsne_nbr_max_k()
    assert cap == 131072 == ops.TSNE_NBR_MAX_N == NR.MAX_N and kmax == 192 == ops.TSNE_NBR_MAX_K == NR.MAX_K
    sup = L.tacorl_tsne_nbr_supported
    assert sup(cap, 32, kmax) == 1 and sup(cap + 1, 16, 120) == 0 and sup(4, 1, 3) == 1 and sup(3, 1, 2) == 0
    assert sup(64, 33, 15) == 0 and sup(64, 0, 15) == 0 and sup(1000, 16, kmax + 1) == 0 and sup(121, 16, 120) == 1
    assert sup(120, 16, 120) == 0 and sup(64, 16, 0) == 0
    assert L.tacorl_tsne_nbr_knn_tile() == 128
    for n in (4, 8192, 8193, 131072):
        assert L.tacorl_tsne_nbr_segment(n) == NR.segment(n)
    assert L.tacorl_tsne_nbr_segment(cap + 1) == 0 and L.tacorl_tsne_nbr_workspace_bytes(cap + 1) == 0
    assert L.tacorl_tsne_nbr_workspace_bytes(3) == 0 and L.tacorl_tsne_nbr_workspace_bytes(64) >= 64 * (32 + 2 + 2 + 1 + 3) * 4
    assert L.tacorl_tsne_nbr_workspace_bytes(cap) < 80 << 20  # nothing of size N x N
    off = (C.c_long * 4)()
    assert L.tacorl_tsne_nbr_workspace_offsets(64, off) == 0 and list(off) == sorted(off) and all(o % 16 == 0 for o in off)
    assert L.tacorl_tsne_nbr_workspace_offsets(cap + 1, off) == -22 and L.tacorl_tsne_nbr_workspace_offsets(64, None) == -22
    assert ops.tsne_nbr_k(40.0) == 120 and ops.tsne_nbr_k(64.0) == 192 and ops.tsne_nbr_k(5.0) == 15
    p = lambda a: C.c_void_p(a)  # noqa: E731  (never dereferenced)
    big = 1 << 40
    A = 4096
    aff = lambda X=A, N=64, D=16, ld=16, perp=5.0, r=A, d=A, c=A, b=A, rp=A, col=A, val=A, capy=2 * 64 * 15, s=A, ws=A, wsb=big: (  # noqa: E731
        L.tacorl_tsne_nbr_affinities(p(X), N, D, ld, perp, p(r), p(d), p(c), p(b), p(rp), p(col), p(val), capy, p(s), p(ws), wsb, None))
    for kw in (dict(N=cap + 1), dict(N=3), dict(D=33), dict(D=0), dict(ld=15), dict(perp=21.4), dict(perp=0.5), dict(perp=float("nan")),
               dict(perp=64.4, N=1000, capy=big), dict(perp=1e30), dict(X=0), dict(r=0), dict(d=0), dict(c=0), dict(b=0), dict(rp=0),
               dict(col=0), dict(val=0), dict(s=0), dict(ws=0), dict(X=4098), dict(col=4098), dict(ws=4100), dict(wsb=128),
               dict(capy=2 * 64 * 15 - 1)):
        assert aff(**kw) == -22, kw
    knn = lambda X=A, N=64, D=16, ld=16, K=15, r=A, d=A: L.tacorl_tsne_nbr_knn(p(X), N, D, ld, K, p(r), p(d), None)  # noqa: E731
    for kw in (dict(N=cap + 1), dict(N=3), dict(D=33), dict(ld=15), dict(K=0), dict(K=64), dict(K=193, N=1000), dict(X=0), dict(r=0),
               dict(d=0), dict(d=4098)):
        assert knn(**kw) == -22, kw
    step = lambda rp=A, col=A, val=A, N=64, Y=A, u=A, g=A, ws=A, wsb=big: L.tacorl_tsne_nbr_step(  # noqa: E731
        p(rp), p(col), p(val), N, p(Y), p(u), p(g), 12.0, 0.5, 200.0, p(ws), wsb, None)
    for kw in (dict(N=cap + 1), dict(N=0), dict(rp=0), dict(col=0), dict(val=0), dict(Y=0), dict(u=0), dict(g=0), dict(ws=0),
               dict(Y=4100), dict(wsb=0)):
        assert step(**kw) == -22, kw
    kl = lambda rp=A, col=A, val=A, Y=A, N=64, out=A, ws=A, wsb=big: L.tacorl_tsne_nbr_kl(  # noqa: E731
        p(rp), p(col), p(val), p(Y), N, p(out), p(ws), wsb, None)
    for kw in (dict(N=cap + 1), dict(rp=0), dict(col=0), dict(val=0), dict(Y=0), dict(out=0), dict(ws=0), dict(wsb=16)):
        assert kl(**kw) == -22, kw


def test_tsneplot_subsample_rule():
    """TSNEPlot._subsample without a GPU: at most max_points rows (None: the neighbour path's cap), drawn without replacement by
    the callback's RandomState(0), sorted, applied to plans and labels alike; nothing is drawn when the epoch fits; and a
    perplexity whose lists the neighbour path does not keep (floor(3 perplexity) > 192) caps the epoch at the dense path's
    8192 rows, whatever max_points says."""
    import torch

    from tacorl_amd import ops
    from tacorl_amd.utils.callbacks.tsne_plot import TSNEPlot

    n = 9000
    plans, labels = torch.arange(n, dtype=torch.float32)[:, None].repeat(1, 3), torch.arange(n)
    for perp, max_points, want in ((40, None, n), (40, 8500, 8500), (40, 10 ** 6, n), (64.4, None, ops.TSNE_MAX_N), (64.4, 8500, ops.TSNE_MAX_N),
                                   (64.4, 5000, 5000), (64, None, n)):
        plot = TSNEPlot(perp, 8, 0.1, 0.3, 5, max_points=max_points)
        p, lab = plot._subsample(plans, labels)
        assert p.shape == (want, 3) and lab.shape == (want,), (perp, max_points)
        if want == n:
            assert p is plans and lab is labels and plot.rng.randint(1 << 30) == np.random.RandomState(0).randint(1 << 30)
        else:
            keep = np.sort(np.random.RandomState(0).choice(n, size=want, replace=False))
            assert np.array_equal(lab.numpy(), keep) and np.array_equal(p[:, 0].numpy(), keep.astype(np.float32))
