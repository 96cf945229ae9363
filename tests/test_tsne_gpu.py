"""The exact t-SNE kernels (tsne_ops.hip) on the GPU against the fp64 restatement of the project's own definition
(tests/tsne_ref.py; include/tacorl_hip.h "exact t-SNE").  Affinities and forces are held to a-priori bounds, short trajectories
to 4 x the deviation of the restatement run in fp32, the whole run to the fixture's recorded fp64 results.  Every case prints
its figures in front of its assertions (tools/tsne_md.py collects them into profiles/tsne.md)."""
import functools

import numpy as np
import pytest
import torch

from tests import tsne_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (16, 63, 64, 65, 255, 257, 1000)
# (N, D, extra columns of the table the rows are sliced from, duplicated rows)
AFF_CASES = [(n, 16, 0, False) for n in NS] + [(257, 1, 0, False), (255, 32, 0, False), (65, 1, 0, False), (65, 16, 5, False),
                                               (257, 16, 0, True)]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the shared references are read-only arrays)


@functools.lru_cache(maxsize=None)
def _affinities(N, D, pad, dup):
    """The kernel's (X, P, beta, status, xn) of a case, computed once and shared (read-only)."""
    from tacorl_amd import ops

    X = R.case_table(N, D, N, duplicates=dup)
    wide = np.full((N, D + pad), 7.0, np.float32)
    wide[:, :D] = X
    Xd = _dev(wide)[:, :D]
    assert Xd.stride(0) == D + pad
    P, beta, status, ws = ops.tsne_affinities(Xd, R.perplexity_for(N))
    torch.cuda.synchronize()
    xn = ops.tsne_workspace_views(ws, N)["xn"].cpu().numpy()
    out = X, P.cpu().numpy(), beta.cpu().numpy(), status.cpu().numpy(), xn
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("N,D,pad,dup", AFF_CASES)
def test_affinities_within_the_allowance(N, D, pad, dup):
    X, P, beta, status, xn = _affinities(N, D, pad, dup)
    perp = R.perplexity_for(N)
    assert status.tolist() == [0, 0]
    # the normalised table
    ref_n, allow_n = R.normalise(X), R.normalise_allowance(X)
    use_n = (np.abs(xn[:, :D] - ref_n) / allow_n).max()
    assert not xn[:, D:].any()
    # entropies and P in fp64 at the kernel's own betas, on the kernel's own (fp32) normalised table
    d = R.sq_dists(xn[:, :D].astype(np.float64))
    b64 = beta.astype(np.float64)
    H = np.array([R.row_entropy(d[i], i, b64[i])[0] for i in range(N)])
    allow_h = np.array([R.entropy_allowance(d[i], i, b64[i], D) for i in range(N)])
    use_h = (np.abs(H - np.log(perp)) / allow_h).max()
    P64 = R.symmetrise(R.cond_rows(d, b64))
    allow_p = R.p_allowance(d, b64, D)
    off = ~np.eye(N, dtype=bool)
    use_p = (np.abs(P - P64)[off] / allow_p[off]).max()
    print(f"tsne affinities N={N} D={D} pad={pad} dup={dup}: allowance use xn {use_n:.3f} H {use_h:.3f} P {use_p:.3f}; "
          f"max |H - log perp| {np.abs(H - np.log(perp)).max():.3g}, sum P - 1 {P.sum(dtype=np.float64) - 1:.3g}")
    assert use_n <= 1 and use_h <= 1 and use_p <= 1
    assert np.array_equal(P.view(np.int32), P.T.view(np.int32))  # symmetric bit for bit
    assert not P.diagonal().any() and (P >= 0).all()
    assert abs(P.sum(dtype=np.float64) - 1) < (N + 8) * R.U * 4


def test_affinities_with_more_than_64_kib_of_distances():
    """N = 4100: four rows of distances take 65.6 KiB of LDS, past the 64 KiB a kernel gets without asking.  64 rows' entropies
    against fp64 at the kernel's betas (P_ij needs every row's fp64 normaliser: left to the sizes above), the matrix's
    symmetry, diagonal and sum."""
    from tacorl_amd import ops

    N, D, perp = 4100, 16, 40.0
    X = R.case_table(N, D, N)
    P, beta, status, ws = ops.tsne_affinities(_dev(X), perp)
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0]
    xn = ops.tsne_workspace_views(ws, N)["xn"].cpu().numpy()[:, :D].astype(np.float64)
    b64, use = beta.cpu().numpy().astype(np.float64), 0.0
    for i in range(0, N, 65):
        d = ((xn - xn[i]) ** 2).sum(1)
        H = R.row_entropy(d, i, b64[i])[0]
        use = max(use, abs(H - np.log(perp)) / R.entropy_allowance(d, i, b64[i], D))
    P = P.cpu().numpy()
    print(f"tsne affinities N={N} D={D}: allowance use H {use:.3f} (64 rows), sum P - 1 {P.sum(dtype=np.float64) - 1:.3g}")
    assert use <= 1
    assert np.array_equal(P.view(np.int32), P.T.view(np.int32)) and not P.diagonal().any() and (P >= 0).all()
    assert abs(P.sum(dtype=np.float64) - 1) < (N + 8) * R.U * 4


def _states(N):
    """[(name, Y, u, gains, exaggeration, momentum)]: the initial state and iteration 300 of the fp64 run (fp32 values)."""
    Y0 = (1e-4 * np.random.RandomState(1000 + N).standard_normal((N, 2))).astype(np.float32)
    mid = R.golden()[f"mid_{N}"]
    return [("init", Y0, np.zeros_like(Y0), np.ones_like(Y0), 12.0, 0.5), ("mid", mid[0], mid[1], mid[2], 1.0, 0.8)]


def _gpu_steps(P, Y, u, g, ex, mom, n):
    """n kernel iterations from the state; returns (Y, u, gains, attr, rep, zrow of the LAST iteration) as host arrays."""
    from tacorl_amd import ops

    Pd, Yd, ud, gd = _dev(P), _dev(Y), _dev(u), _dev(g)
    ws = ops.tsne_workspace(len(P), DEV)
    for _ in range(n):
        ops.tsne_step(Pd, Yd, ud, gd, ex, mom, 200.0, ws)
    torch.cuda.synchronize()
    v = ops.tsne_workspace_views(ws, len(P))
    return [t.cpu().numpy() for t in (Yd, ud, gd, v["attr"], v["rep"], v["zrow"])]


@pytest.mark.parametrize("N", NS)
def test_forces_within_the_a_priori_bound(N):
    P = _affinities(N, 16, 0, False)[1]
    P64 = P.astype(np.float64)
    for name, Y, u, g, ex, mom in _states(N):
        got = _gpu_steps(P, Y, u, g, ex, mom, 1)
        attr, rep, zi, s_attr, s_rep, s_z = R.forces(P64, Y.astype(np.float64))
        use = [(np.abs(a - b) / np.maximum(R.sum_bound(N, s), 1e-300)).max()
               for a, b, s in ((got[3], attr, s_attr), (got[4], rep, s_rep), (got[5], zi, s_z))]
        print(f"tsne forces N={N} {name}: bound use attr {use[0]:.3f} rep {use[1]:.3f} Z_i {use[2]:.3f}")
        assert max(use) <= 1
        again = _gpu_steps(P, Y, u, g, ex, mom, 1)
        for a, b in zip(got, again):  # two launches: identical bits, the updated state included
            assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("N", NS)
def test_three_steps_follow_the_fp64_restatement(N):
    """Tolerance: 4 x the deviation (Frobenius norm over Y, and over u) of the restatement run in fp32 on the same problem -
    the factor the MLP gradient tests use.  The fp32 run takes every sum in the order the definition states
    (tsne_ref.step_in_kernel_order): at N = 16 the first iterations amplify a rounding difference several thousand times, and
    an fp32 run that merely sums in another order deviates by a different few ulps (measured: kernel 1.5e-4 in u against
    2.7e-5 of a NumPy-order fp32 run, |u| = 81).  Not extended past a handful of steps: the sign rule of the gains makes fp32 and
    fp64 runs part company by about iteration 20."""
    P = _affinities(N, 16, 0, False)[1]
    for name, Y, u, g, ex, mom in _states(N):
        ref = {}
        for dt in (np.float64, np.float32):
            s = (Y.astype(dt), u.astype(dt), g.astype(dt))
            for _ in range(3):
                s = (R.step if dt is np.float64 else R.step_in_kernel_order)(P.astype(dt), *s, ex, mom, 200.0)
            assert s[0].dtype == dt
            ref[dt] = s
        got = _gpu_steps(P, Y, u, g, ex, mom, 3)
        for k, what in ((0, "Y"), (1, "u")):
            dev32 = np.linalg.norm(ref[np.float32][k].astype(np.float64) - ref[np.float64][k])
            devk = np.linalg.norm(got[k].astype(np.float64) - ref[np.float64][k])
            print(f"tsne trajectory N={N} {name} {what}: kernel {devk:.3g}, fp32 restatement {dev32:.3g}, "
                  f"|{what}| {np.linalg.norm(ref[np.float64][k]):.3g}")
            assert devk <= 4 * dev32


def test_kl_against_fp64():
    from tacorl_amd import ops

    N = 257
    P = _affinities(N, 16, 0, False)[1]
    Y = R.golden()[f"mid_{N}"][0]
    out = ops.tsne_kl(_dev(P), _dev(Y), ops.tsne_workspace(N, DEV))
    got = float(out.item())
    P64, Y64 = P.astype(np.float64), Y.astype(np.float64)
    q = ((Y64[:, None] - Y64[None]) ** 2).sum(-1)
    w = 1 / (1 + q)
    np.fill_diagonal(w, 0)
    pos = P64 > 0
    mag = (P64[pos] * (np.abs(np.log(P64[pos])) + np.log1p(q[pos]))).sum() + (abs(np.log(w.sum())) + 1) * P64.sum()
    want = R.kl(P64, Y64)
    print(f"tsne kl N={N}: kernel {got:.7g} fp64 {want:.7g}, bound use {abs(got - want) / R.sum_bound(N, mag):.3f}")
    assert abs(got - want) <= R.sum_bound(N, mag)


def test_whole_run_separates_the_fixture_clusters():
    from tacorl_amd.evaluation.tsne import tsne_embed

    G = R.golden()
    Y, kl = tsne_embed(_dev(G["X"]), perplexity=float(G["perplexity"]), init=_dev(G["inits"][0].astype(np.float32)),
                       return_kl=True)
    assert Y.shape == (240, 2) and Y.dtype == torch.float32 and Y.is_cuda
    acc = R.knn_accuracy(Y.cpu().numpy(), G["labels"])
    limit = G["kl"].max() + (G["kl"].max() - G["kl"].min())
    print(f"tsne whole run: KL {kl:.4f} (fp64 runs {G['kl'].min():.4f} .. {G['kl'].max():.4f}, limit {limit:.4f}), 5-NN accuracy {acc:.3f}")
    assert acc >= 0.98 and kl <= limit
    # a generator-seeded start gives the same picture, and repeats
    gen = torch.Generator(device=DEV).manual_seed(3)
    Y1 = tsne_embed(_dev(G["X"]).view(6, 40, 16), perplexity=30.0, generator=gen)
    Y2 = tsne_embed(_dev(G["X"]), perplexity=30.0, generator=torch.Generator(device=DEV).manual_seed(3))
    assert torch.equal(Y1, Y2) and R.knn_accuracy(Y1.cpu().numpy(), G["labels"]) >= 0.98


def test_refusals():
    from tacorl_amd import _lib, ops
    from tacorl_amd.evaluation.tsne import tsne_embed

    E = _lib.TacorlHipError
    with pytest.raises(E):
        tsne_embed(torch.zeros(ops.TSNE_MAX_N + 1, 2, device=DEV), perplexity=5.0)
    with pytest.raises(E):
        tsne_embed(torch.randn(64, 33, device=DEV), perplexity=5.0)
    with pytest.raises(E):
        tsne_embed(torch.randn(16, 4, device=DEV), perplexity=5.1)  # 3 * 5.1 > 15
    with pytest.raises(E):
        tsne_embed(torch.randn(16, 4), perplexity=5.0)              # a host tensor: there is no host path
    with pytest.raises(ValueError):
        tsne_embed(torch.full((32, 8), 0.25, device=DEV), perplexity=5.0, n_iter=1)
    X = torch.randn(16, 4, device=DEV)
    with pytest.raises(E):
        ops.tsne_affinities(X, 5.0, ws=torch.empty(64, dtype=torch.uint8, device=DEV))  # a short workspace
    L = _lib.lib()
    P, b, s, ws = ops.tsne_affinities(X, 5.0)
    p = _lib.ptr
    assert L.tacorl_tsne_affinities(None, 16, 4, 4, 5.0, p(P), p(b), p(s), p(ws), ws.numel(), None) == -22
    assert L.tacorl_tsne_affinities(p(X), 16, 4, 3, 5.0, p(P), p(b), p(s), p(ws), ws.numel(), None) == -22  # ld < D
    assert L.tacorl_tsne_step(p(P), 16, None, p(b), p(b), 1.0, 0.5, 200.0, p(ws), ws.numel(), None) == -22
    assert L.tacorl_tsne_kl(p(P), p(X), 16, None, p(ws), ws.numel(), None) == -22
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ the callbacks on a real module
def _playlmp():
    from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP
    from tests.golden_util import Golden
    from tests.test_step_gpu import ACTOR

    g = Golden("playlmp")
    cams, c = sorted(g.cams), g.cfg
    pr = dict(num_heads=8, num_layers=2, encoder_hidden_size=2048, fc_hidden_size=4096, latent_plan_dim=c["latent"],
              min_std=1e-4, dropout_p=0.0, max_position_embeddings=c["T"])
    ad = dict(n_mixtures=10, num_layers=2, hidden_size=2048, out_features=7, num_classes=10,
              latent_plan_dim=c["latent"], rnn_model="rnn_decoder", include_goal=False)
    mod = PlayLMP(plan_proposal=ACTOR, plan_recognition=pr, action_decoder=ad, plan_proposal_obs_modalities=cams,
                  plan_proposal_goal_modalities=cams, plan_recognition_modalities=cams, action_decoder_modalities=cams,
                  real_world=True, lr=1e-4, kl_beta=1e-3, device=DEV, compute_dtype="f32")
    mod.load_state_dict(g.params(), strict=False)
    return mod, g


def test_callbacks_through_minitrainer_on_playlmp():
    """Two validation batches of a PlayLMP built from the `playlmp` golden through MiniTrainer with the reference's callback
    group: TSNEPlot maps the plans it samples from last_plan_proposal(), and the KL schedule's beta reaches the (captured)
    step - kl_loss_scaled / kl_loss is the epoch's beta."""
    from tacorl_amd.lightning import MiniTrainer
    from tacorl_amd.utils.callbacks.kl_callbacks import KLLinearSchedule
    from tacorl_amd.utils.callbacks.tsne_plot import TSNEPlot

    mod, g = _playlmp()
    mod.enable_graph()
    batch = g.batch(0)
    B, A = batch["actions"].shape[0], g.cfg["latent"]
    n = 2 * B
    plot = TSNEPlot(perplexity=min(5.0, 0.9 * (n - 1) / 3), n_jobs=8, plot_percentage=1.0, opacity=0.3, marker_size=5)
    seen = []

    class Watch:
        def on_train_batch_end(self, trainer, pl_module, outputs, batch, batch_idx, unused=0):
            seen.append((pl_module.kl_beta, pl_module.logged["train/kl_loss"], pl_module.logged["train/kl_loss_scaled"]))

        def on_validation_batch_end(self, trainer, pl_module, outputs, batch, batch_idx, dataloader_idx=0):
            d = pl_module.last_plan_proposal()
            head = pl_module.pact[pl_module.p_yoff: pl_module.p_yoff + B * 2 * A].view(B, 2 * A)
            assert torch.equal(d.normal_mean, head[:, :A].clamp(-9.0, 9.0)) and torch.equal(d.mean, torch.tanh(d.normal_mean))
            assert torch.equal(d.stddev, head[:, A:].clamp(-5.0, 2.0).exp()) and d.stddev.shape == (B, A)

    tr = MiniTrainer(max_epochs=3, log_every_n_steps=1, callbacks=[KLLinearSchedule(0, 2, 0.1), Watch(), plot])
    tr.fit(mod, [batch], [batch, batch])
    torch.cuda.synchronize()
    print("tsne callback: (beta, kl, kl_scaled) per epoch", seen, "map KL", plot.last["kl"])
    assert [s[0] for s in seen] == [0.0, 0.05, 0.1]
    for beta, kl, scaled in seen:
        assert kl > 0 and abs(scaled - beta * kl) <= 1e-5 * beta * kl
    last = plot.last
    assert last["x_tsne"].shape == (n, 2) and np.isfinite(last["x_tsne"]).all() and np.isfinite(last["kl"])
    assert last["labels"].tolist() == [-1] * n and last["step"] == 3 and len(last["shown"]) == min(n, 100)
