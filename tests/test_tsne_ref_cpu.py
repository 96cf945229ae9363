"""The fp64 restatement of the project's exact t-SNE (tests/tsne_ref.py) and the allowances the GPU tests use, checked without a
GPU: the fixture (tests/golden/tsne_clusters.npz, tools/gen_tsne_fixture.py) regenerates, the definition has the properties it
must have, the a-priori bounds hold for an fp32 evaluation and are discriminating, and the entry points refuse bad arguments
before they touch a device."""
import ctypes as C

import numpy as np
import pytest

from tests import tsne_ref as R

NS = (16, 63, 257, 1000)


@pytest.fixture(scope="module")
def fixture_affinities():
    G = R.golden()
    P, betas, capped, d = R.affinities(G["X"], float(G["perplexity"]))
    for a in (P, betas, d):
        a.setflags(write=False)
    return G, P, betas, capped, d


def test_fixture_table_is_the_generators():
    G = R.golden()
    X, labels = R.clusters()
    assert np.array_equal(G["X"], X) and np.array_equal(G["labels"], labels) and X.shape == (240, 16) and float(G["perplexity"]) == 30.0
    assert G["inits"].shape == (8, 240, 2) and 0.5e-4 < G["inits"].std() < 2e-4
    for N in (16, 63, 64, 65, 255, 257, 1000):
        mid = G[f"mid_{N}"]
        assert mid.shape == (3, N, 2) and mid.dtype == np.float32 and mid[2].min() >= 0.01 and mid[2].max() > 2  # spread gains


def test_entropy_condition_and_definition_properties(fixture_affinities):
    G, P, betas, capped, d = fixture_affinities
    assert capped == 0
    H = np.array([R.row_entropy(d[i], i, betas[i])[0] for i in range(len(d))])
    assert np.abs(H - np.log(30.0)).max() < 1e-5
    # the unshifted entropy -sum p log p of p_{j|i} = exp(-beta d_ij) / sum_k exp(-beta d_ik) is the same number
    i = 7
    e = np.exp(-betas[i] * np.delete(d[i], i))
    p = e / e.sum()
    assert abs(-(p * np.log(p)).sum() - H[i]) < 1e-12
    assert np.array_equal(P, P.T) and not P.diagonal().any() and abs(P.sum() - 1) < 1e-12 and (P >= 0).all()


def test_fp64_run_reproduces_the_recorded_results(fixture_affinities):
    G, P, *_ = fixture_affinities
    assert abs(R.kl(P, G["inits"][0]) - G["kl0"][0]) < 1e-9 and 2.0 < G["kl0"][0] < 2.1
    assert G["kl"].min() > 0.125 and G["kl"].max() < 0.135 and (G["acc"] == 1.0).all()
    Y = R.run(P, G["inits"][0])
    assert abs(R.kl(P, Y) - G["kl"][0]) < 1e-6 and R.knn_accuracy(Y, G["labels"]) == 1.0


def test_forces_are_translation_invariant():
    G = R.golden()
    P = R.affinities(R.case_table(63, 16, 63), 5.0)[0]
    Y = G["mid_63"][0].astype(np.float64)
    a = R.forces(P, Y)[:3]
    b = R.forces(P, Y + np.array([3.5, -1.25]))[:3]
    for x, y in zip(a, b):
        assert np.abs(x - y).max() <= 1e-12 * max(1.0, np.abs(x).max())


@pytest.mark.parametrize("N", (16, 257, 1000))
def test_the_ordered_statement_is_the_same_function(N):
    """step_in_kernel_order differs from step in the order of its sums only: in fp64 the two agree to rounding."""
    G = R.golden()
    P = R.affinities(R.case_table(N, 16, N), R.perplexity_for(N))[0]
    s = tuple(a.astype(np.float64) for a in G[f"mid_{N}"])
    a, b = R.step(P, *s, 1.0, 0.8, 200.0), R.step_in_kernel_order(P, *s, 1.0, 0.8, 200.0)
    assert np.array_equal(a[2], b[2])
    for x, y in zip(a[:2], b[:2]):
        assert np.abs(x - y).max() <= 1e-10 * np.abs(x).max()


def _states(N):
    G = R.golden()
    Y0 = (1e-4 * np.random.RandomState(1000 + N).standard_normal((N, 2))).astype(np.float32)
    return [("init", Y0)] + ([("mid", G[f"mid_{N}"][0])] if f"mid_{N}" in G else [])


@pytest.mark.parametrize("N", NS)
def test_force_bound_holds_for_fp32_and_is_discriminating(N):
    """(N + 8) u sum|term| per row and component: an fp32 evaluation with a sequential fp32 sum stays inside it; leaving one j
    out of one row's sums (a change of |term_ij| in each sum) leaves it for at least 90 % of the pairs (i, j) at the initial
    state.  At the mid-run state the far pairs' terms are below the bound by construction (w_ij ~ 1e-4 of the row's sum):
    its fraction is printed, not asserted."""
    P32 = R.affinities(R.case_table(N, 16, N), R.perplexity_for(N))[0].astype(np.float32)
    P64 = P32.astype(np.float64)
    for name, Y in _states(N):
        attr, rep, zi, s_attr, s_rep, s_z = R.forces(P64, Y.astype(np.float64))
        diff = Y[:, None, :] - Y[None, :, :]
        w = np.float32(1) / (np.float32(1) + (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]))
        np.fill_diagonal(w, 0)
        ta, tr = (P32 * w)[:, :, None] * diff, (w * w)[:, :, None] * diff
        assert ta.dtype == np.float32
        seq = lambda t: np.cumsum(t, axis=1, dtype=np.float32)[:, -1]  # noqa: E731
        use = max((np.abs(seq(t) - r) / R.sum_bound(N, s)).max() for t, r, s in ((ta, attr, s_attr), (tr, rep, s_rep), (w, zi, s_z)))
        assert use <= 1
        off = ~np.eye(N, dtype=bool)
        caught = ((np.abs(ta.astype(np.float64)) > 2 * R.sum_bound(N, s_attr)[:, None, :]).any(-1)
                  | (np.abs(tr.astype(np.float64)) > 2 * R.sum_bound(N, s_rep)[:, None, :]).any(-1)
                  | (w.astype(np.float64) > 2 * R.sum_bound(N, s_z)[:, None]))
        frac = caught[off].mean()
        print(f"N={N} {name}: fp32 sequential sum uses {use:.3f} of the bound; a dropped term leaves it for {100 * frac:.1f} % of (i, j)")
        if name == "init":
            assert frac >= 0.90


@pytest.mark.parametrize("N,D", [(16, 16), (63, 1), (257, 16), (257, 32), (1000, 16)])
def test_affinity_allowances_hold_for_fp32_and_are_discriminating(N, D):
    """The fp32 run of the restatement (its own betas) is inside the allowances for H_i and P_ij, evaluated in fp64 at those
    betas on the fp32-normalised table; a beta off by one bisection step at step 10 moves H_i, and dropping p_{i|j} from one
    element moves P_ij, by at least 10 x the allowance."""
    X = R.case_table(N, D, N)
    perp = R.perplexity_for(N)
    xn32 = R.normalise(X, np.float32)
    assert xn32.dtype == np.float32 and (np.abs(xn32 - R.normalise(X)) <= R.normalise_allowance(X)).all()
    d32 = R.sq_dists(xn32)
    d = R.sq_dists(xn32.astype(np.float64))
    rows = range(N) if N <= 300 else range(0, N, 7)
    betas, ratios_h = np.ones(N), []
    for i in range(N):
        trace = []
        b, capped = R.search_beta(d32[i], i, perp, trace)
        assert not capped and b.dtype == np.float32
        betas[i] = b
        if i in rows:
            allow = R.entropy_allowance(d[i], i, betas[i], D)
            H = R.row_entropy(d[i], i, betas[i])[0]
            assert abs(H - np.log(perp)) <= allow
            if len(trace) < 12:  # (a search that happened to converge before step 10 has no such fault)
                continue
            t9, t10 = float(trace[9]), float(trace[10])
            # the wrong branch at step 10: the midpoint of the half the final beta is NOT in (at least |t10 - t9| / 2 away)
            wrong = t10 - (t10 - t9) / 2 if (betas[i] - t10) * (t10 - t9) > 0 else t10 + (t10 - t9) / 2
            ratios_h.append(abs(R.row_entropy(d[i], i, wrong)[0] - np.log(perp)) / allow)
    c32 = R.cond_rows(d32, betas.astype(np.float32))
    assert c32.dtype == np.float32
    P32 = R.symmetrise(c32)
    c64 = R.cond_rows(d, betas)
    P64, allow_p = R.symmetrise(c64), R.p_allowance(d, betas, D)
    assert (np.abs(P32 - P64) <= allow_p).all()
    j = c64.argmax(1)  # each row's largest conditional entry: P_ij without its p_{j|i} half
    i = np.arange(N)
    ratios_p = (c64[i, j] / (2 * N)) / allow_p[i, j]
    print(f"N={N} D={D}: fault / allowance: H min {min(ratios_h):.1f}, P min {ratios_p.min():.1f}; "
          f"allowance H max {max(R.entropy_allowance(d[r], r, betas[r], D) for r in rows):.3g}")
    assert len(ratios_h) >= 0.8 * len(rows) and min(ratios_h) >= 10 and ratios_p.min() >= 10


def test_entry_points_refuse_before_any_launch():
    """No GPU here: every call below must come back from its argument checks."""
    from tacorl_amd import _lib

    L = _lib.lib()
    cap = L.tacorl_tsne_max_n()
    assert cap == 8192 and L.tacorl_tsne_supported(cap, 32) == 1 and L.tacorl_tsne_supported(cap + 1, 16) == 0
    assert L.tacorl_tsne_supported(64, 33) == 0 and L.tacorl_tsne_supported(64, 0) == 0 and L.tacorl_tsne_supported(3, 2) == 0
    assert L.tacorl_tsne_workspace_bytes(cap + 1) == 0 and L.tacorl_tsne_workspace_bytes(64) >= 64 * (32 + 2 + 2 + 1) * 4
    off = (C.c_long * 4)()
    assert L.tacorl_tsne_workspace_offsets(64, off) == 0 and list(off) == sorted(off) and all(o % 16 == 0 for o in off)
    assert off[3] + 64 * 4 <= L.tacorl_tsne_workspace_bytes(64)
    assert L.tacorl_tsne_workspace_offsets(cap + 1, off) == -22 and L.tacorl_tsne_workspace_offsets(64, None) == -22
    p = lambda a: C.c_void_p(a)  # noqa: E731  (never dereferenced)
    big = 1 << 40
    aff = lambda X=4096, N=64, D=16, ld=16, perp=5.0, P=8192, b=4096, s=4096, ws=4096, wsb=big: L.tacorl_tsne_affinities(  # noqa: E731
        p(X), N, D, ld, perp, p(P), p(b), p(s), p(ws), wsb, None)
    for kw in (dict(N=cap + 1), dict(D=33), dict(D=0), dict(ld=15), dict(perp=21.1), dict(perp=0.5), dict(perp=float("nan")),
               dict(X=0), dict(P=0), dict(b=0), dict(s=0), dict(ws=0), dict(X=4098), dict(P=8196), dict(ws=4100), dict(wsb=128), dict(N=3)):
        assert aff(**kw) == -22, kw
    step = lambda P=8192, N=64, Y=4096, u=4096, g=4096, ws=4096, wsb=big: L.tacorl_tsne_step(  # noqa: E731
        p(P), N, p(Y), p(u), p(g), 12.0, 0.5, 200.0, p(ws), wsb, None)
    for kw in (dict(N=cap + 1), dict(N=0), dict(P=0), dict(Y=0), dict(u=0), dict(g=0), dict(ws=0), dict(Y=4100), dict(wsb=0)):
        assert step(**kw) == -22, kw
    kl = lambda P=8192, Y=4096, N=64, out=4096, ws=4096, wsb=big: L.tacorl_tsne_kl(p(P), p(Y), N, p(out), p(ws), wsb, None)  # noqa: E731
    for kw in (dict(N=cap + 1), dict(P=0), dict(Y=0), dict(out=0), dict(ws=0), dict(wsb=16)):
        assert kl(**kw) == -22, kw
