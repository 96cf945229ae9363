"""Full-size checks (BASELINE configs[1]: B=256, T=16, 84x84, latent 16, n=4, Q phase) of the TACORL
step on the GPU: direct comparison with the oracle in exact-fp32 mode, plus the size-independent
properties the step offers - run-to-run bit determinism, batch-mean linearity of the critic gradients
(full batch == mean of the two half batches, the property the data-parallel sharding relies on), and
fused-launch == per-layer encoder in bf16 mode."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

B, T, H, W = 256, 16, 84, 84


def _mod(compute, graph=False, batch=B):
    import bench

    torch.manual_seed(0)
    mod = bench.build_module(torch.device("cuda:0"), compute, T, 1)
    if graph:
        mod.enable_graph()
    return mod


def _batch(n=B, seed=77):
    import bench

    return bench.synth_batch(n, T, H, W, torch.device("cuda:0"), seed)


def _logs(mod):
    torch.cuda.synchronize()
    return {k.split("/", 1)[1]: float(v) for k, v in mod.logged.items()}


def _noise(mod):
    nz = {k: v.clone() for k, v in mod.engine.noise.items()}
    nz["eps_pr"] = mod.eps_pr.clone()
    return nz


def _oracle_inputs(mod):
    from oracle import tacorl_oracle as O

    cams = ["rgb_static"]
    spec = O.ACSpec(cams=cams, goal_cams=cams, action_dim=16, n=4, discount=0.95, actor_lr=1e-4, critic_lr=3e-4,
                    deterministic_backup=True, reward_scale=10.0, bc_epochs=5, with_lagrange=True,
                    discrete_gripper=False, target_entropy=-7.0, finetune_action_decoder=False, ac_cams=cams,
                    pr_cams=cams)
    skip = ("one_hot_embedding_eye", "ones", "gripper_bounds", "action_max_bound", "action_min_bound")
    P = {k: v.detach().cpu().clone().contiguous() for k, v in mod.state_dict().items()
         if v.dtype == torch.float32 and not any(k.endswith(s) for s in skip)}
    O.require_grad_(P, frozen_prefixes=("perceptual_encoder.", "plan_recognition."))
    return O, spec, P


def _cpu(x):
    if isinstance(x, dict):
        return {k: _cpu(v) for k, v in x.items()}
    return x.cpu() if torch.is_tensor(x) else x


def test_fullsize_f32_step_matches_oracle():
    """B=256 exact-fp32 step vs the CPU oracle on the same parameters, batch and noise: every logged
    loss and the sampled latent plans within 1e-4 rel (north-star tolerance), gradients within 1e-3."""
    mod = _mod("f32")
    O, spec, P = _oracle_inputs(mod)
    opts = O.make_opts(P, spec)
    batch = _batch()
    mod.logged = {}
    mod.training_step(batch)
    got, nz = _logs(mod), _cpu(_noise(mod))
    ologs, oplan, ograds = O.tacorl_step(P, opts, spec, _cpu(batch), nz, 5)
    bad = []
    for k, v in ologs.items():
        v = float(v)
        if k in got and abs(got[k] - v) > 1e-4 * max(abs(v), 1e-3):
            bad.append(f"{k}: hip {got[k]:.8g} oracle {v:.8g}")
    assert len(set(ologs) & set(got)) >= 8, (sorted(ologs), sorted(got))
    e = (mod.plan.cpu() - oplan).norm() / oplan.norm()
    if e > 1e-4:
        bad.append(f"latent plan relerr {e:.3g}")
    grads = mod.named_gradients()
    for k, g in ograds.items():
        if k in grads and g is not None:
            d = (grads[k].cpu().reshape(g.shape) - g).norm() / max(g.norm().item(), 1e-12)
            if d > 1e-3 and g.norm() > 1e-6:
                bad.append(f"grad {k}: relerr {d:.3g}")
    assert not bad, "\n".join(bad[:30])


@pytest.mark.parametrize("graph", [False, True])
def test_fullsize_bf16_bit_deterministic(graph):
    """Two runs from the same seed (three optimiser steps each, side streams and graph branches
    included) end in bit-identical parameters: no atomics, fixed reduction orders."""
    ends = []
    for _ in range(2):
        mod = _mod("bf16", graph)
        batch = _batch()
        torch.manual_seed(5)
        for _ in range(3 if not graph else 5):
            mod.training_step(batch)
        torch.cuda.synchronize()
        ends.append({k: v.detach().clone() for k, v in mod.state_dict().items()})
        logs = mod.engine.metrics()
        assert all(v == v for v in logs.values())
    diff = [k for k in ends[0] if not torch.equal(ends[0][k], ends[1][k])]
    assert not diff, diff[:10]


def test_fullsize_critic_grads_are_batch_means():
    """Gradient linearity at full size: critic gradients of the 256-sample step equal the mean of the
    two 128-sample half steps (same parameters, noise sliced by sample).  With deterministic_backup
    the critic loss does not read alpha, so this holds to fp32 re-association error."""
    from tacorl_amd.dist import shard_batch, shard_noise

    full = _mod("f32")
    batch = _batch()
    full.training_step(batch)
    torch.cuda.synchronize()
    nz = _noise(full)
    gfull = {k: v.clone() for k, v in full.named_gradients().items() if k.startswith(("q1.", "q2."))}
    acc = {k: torch.zeros_like(v) for k, v in gfull.items()}
    for r in range(2):
        half = _mod("f32")
        half.training_step(shard_batch(batch, r, 2), noise=shard_noise(nz, r, 2, 4))
        torch.cuda.synchronize()
        for k, v in half.named_gradients().items():
            if k in acc:
                acc[k] += 0.5 * v
        del half
    bad = []
    for k, g in gfull.items():
        d = (acc[k] - g).norm() / max(g.norm().item(), 1e-12)
        if d > 5e-4 and g.norm() > 1e-6:
            bad.append(f"{k}: {d:.3g}")
    assert gfull and not bad, bad[:20]


def test_fullsize_fused_encoder_equals_per_layer():
    """bf16 mode: the single fused encoder launch (27*B images) and the per-layer kernels give the same
    step - same bf16 operand rounding, different fp32 accumulation order only."""
    res = []
    for fused in (True, False):
        mod = _mod("bf16")
        mod.engine.use_fused = fused
        batch = _batch()
        torch.manual_seed(9)
        mod.logged = {}
        mod.training_step(batch)
        res.append((_logs(mod), mod.plan.clone(), {k: v.clone() for k, v in mod.named_gradients().items()}))
    (la, pa, ga), (lb, pb, gb) = res
    assert torch.equal(pa, pb) or (pa - pb).norm() / pb.norm() < 2e-3
    bad = [f"{k}: {la[k]:.6g} vs {lb[k]:.6g}" for k in la if abs(la[k] - lb[k]) > 3e-3 * max(abs(lb[k]), 1e-2)]
    for k in ga:
        n = gb[k].norm().item()
        if n > 1e-6:
            cos = torch.dot(ga[k].flatten(), gb[k].flatten()).item() / (ga[k].norm().item() * n)
            if cos < 0.995:
                bad.append(f"grad {k}: cosine {cos:.4f}")
    assert not bad, "\n".join(bad[:20])


def test_fullsize_cql_baseline_c5():
    """BASELINE configs C5: CQL_Offline, discrete gripper, A=7, n=32 action samples, B=1024, 84x84, bf16 -
    runs (hipGraph), losses finite, second step changes the parameters."""
    from tacorl_amd import synth
    from tacorl_amd.modules.cql.cql_offline_lightning import CQL_Offline

    dev = torch.device("cuda:0")
    Bc = 1024
    mod = CQL_Offline(actor={"policy": {"num_layers": 3, "hidden_dim": 256}, "discrete_gripper": True},
                      critic={"q_network": {"num_layers": 3, "hidden_dim": 256, "last_layer_activation": "Identity"}},
                      real_world=True, obs_modalities=["rgb_static"], goal_modalities=["rgb_static"], action_dim=7, device="cuda:0",
                      compute_dtype="bf16", image_dtype="bf16", discount=0.99, actor_lr=1e-4, critic_lr=3e-4,
                      conservative_weight=1.0, n_action_samples=32, with_lagrange=True, reward_scale=10.0,
                      deterministic_backup=False, bc_epochs=5)
    mod.current_epoch = 5
    batch = synth.make_transition_batch(7, Bc, {"rgb_static": (84, 84)})
    batch = {k: ({kk: ({c: t.to(dev) for c, t in vv.items()}) for kk, vv in v.items()} if isinstance(v, dict) else v.to(dev))
             for k, v in batch.items()}
    mod.enable_graph()
    before = mod.engine.q1.param.clone()
    for _ in range(3):
        mod.training_step(batch, 0)
    torch.cuda.synchronize()
    logs = mod.engine.metrics()
    assert all(v == v and abs(v) < 1e30 for v in logs.values()), logs
    assert not torch.equal(before, mod.engine.q1.param)


def test_fullsize_cql_baseline_c5_f32_matches_oracle():
    """BASELINE configs C5 at its stated size (CQL_Offline, discrete gripper, A=7, n=32 action samples in the
    logsumexp, B=1024, 84x84) in exact-fp32 mode against the CPU oracle on the same parameters, batch and noise:
    every logged loss within 1e-4 rel (north-star tolerance), gradients within 1e-3."""
    from oracle import tacorl_oracle as O
    from tacorl_amd import synth
    from tacorl_amd.modules.cql.cql_offline_lightning import CQL_Offline

    dev = torch.device("cuda:0")
    Bc, n = 1024, 32
    torch.manual_seed(3)
    mod = CQL_Offline(actor={"policy": {"num_layers": 3, "hidden_dim": 256}, "discrete_gripper": True},
                      critic={"q_network": {"num_layers": 3, "hidden_dim": 256, "last_layer_activation": "Identity"}},
                      real_world=True, obs_modalities=["rgb_static"], goal_modalities=["rgb_static"], action_dim=7, device="cuda:0",
                      compute_dtype="f32", image_dtype="f32", discount=0.99, actor_lr=1e-4, critic_lr=3e-4,
                      conservative_weight=1.0, n_action_samples=n, with_lagrange=True, reward_scale=10.0,
                      deterministic_backup=False, bc_epochs=5)
    mod.current_epoch = 5
    from tacorl_amd.init import init_views_
    for blk in (mod.engine.actor, mod.engine.q1, mod.engine.q2):
        init_views_(blk.views)
    mod.sync_targets()
    cams = ["rgb_static"]
    spec = O.ACSpec(cams=cams, goal_cams=cams, action_dim=7, n=n, discount=0.99, actor_lr=1e-4, critic_lr=3e-4,
                    deterministic_backup=False, reward_scale=10.0, bc_epochs=5, with_lagrange=True,
                    discrete_gripper=True, target_entropy=-7.0)
    P = {k: v.detach().cpu().clone().contiguous() for k, v in mod.state_dict().items()}
    O.require_grad_(P)
    opts = O.make_opts(P, spec)
    batch = synth.make_transition_batch(7, Bc, {"rgb_static": (84, 84)})
    mod.logged = {}
    mod.training_step(_to_dev(batch, dev), 0)
    torch.cuda.synchronize()
    got = {k.split("/", 1)[1]: float(v) for k, v in mod.logged.items()}
    nz = {k: v.detach().cpu().clone() for k, v in mod.engine.noise.items()}
    ologs, ograds = O.cql_step(P, opts, spec, batch, nz, 5)
    bad = [f"{k}: hip {got[k]:.8g} oracle {float(v):.8g}" for k, v in ologs.items()
           if k in got and abs(got[k] - float(v)) > 1e-4 * max(abs(float(v)), 1e-3)]
    assert len(set(ologs) & set(got)) >= 8, (sorted(ologs), sorted(got))
    grads = mod.named_gradients()
    for k, g in ograds.items():
        if k in grads and g is not None and g.norm() > 1e-6:
            d = (grads[k].cpu().reshape(g.shape) - g).norm() / g.norm()
            if d > 1e-3:
                bad.append(f"grad {k}: relerr {d:.3g}")
    assert not bad, "\n".join(bad[:30])


def _to_dev(x, dev):
    if isinstance(x, dict):
        return {k: _to_dev(v, dev) for k, v in x.items()}
    return x.to(dev) if torch.is_tensor(x) else x


@pytest.mark.parametrize("compute", ["bf16", "f32"])
def test_uint8_frames_equal_transformed_fp32_frames(compute):
    """the dataset's uint8 HWC frames handed to the step as they are (normalised on the GPU:
    ToTensor + Normalize(0.5, 0.5)) must give bit-identical image buffers, and so an identical step, to the
    reference route (the same frames transformed to fp32 CHW on the host side)."""
    dev = torch.device("cuda:0")
    n = 32
    g = torch.Generator(device=dev).manual_seed(5)
    s8 = torch.randint(0, 256, (n, T, H, W, 3), device=dev, dtype=torch.uint8, generator=g)
    g8 = torch.randint(0, 256, (n, H, W, 3), device=dev, dtype=torch.uint8, generator=g)
    base = _batch(n)
    # torchvision ToTensor (x.div(255)) + Normalize(0.5, 0.5) ((t - 0.5) / 0.5), on the CPU as the dataloader workers
    # run them (a GPU tensor / python scalar is computed as x * (1 / 255) by torch: 1 ulp off the true quotient)
    tf = lambda x: ((x.cpu().float().div(255) - 0.5) / 0.5).to(dev)  # noqa: E731
    b32 = dict(base, states={"rgb_static": tf(s8).permute(0, 1, 4, 2, 3).contiguous()},
               goal={"rgb_static": tf(g8).permute(0, 3, 1, 2).contiguous()})
    b8 = dict(base, states={"rgb_static": s8}, goal={"rgb_static": g8})
    ma, mb = _mod(compute), _mod(compute)
    ma.training_step(b32)
    nz = _noise(ma)
    mb.training_step(b8, noise=nz)
    torch.cuda.synchronize()
    assert torch.equal(ma.frames["rgb_static"], mb.frames["rgb_static"])
    assert torch.equal(ma.engine.X3["rgb_static"], mb.engine.X3["rgb_static"])
    la, lb = _logs(ma), _logs(mb)
    assert la == lb, (la, lb)
    for (ka, va), (kb, vb) in zip(sorted(ma.state_dict().items()), sorted(mb.state_dict().items())):
        assert ka == kb and torch.equal(va, vb), ka


def test_uint8_frames_cql_offline_and_playlmp():
    """The same equality for the other two module classes' staging: CQL_Offline (engine.load_images) and
    PlayLMP (window frames): uint8 HWC frames vs the host-transformed fp32 CHW route -> identical image buffers."""
    from tacorl_amd.modules.cql.cql_offline_lightning import CQL_Offline
    from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(9)
    tf = lambda x: ((x.cpu().float().div(255) - 0.5) / 0.5).to(dev)  # noqa: E731  ToTensor + Normalize(0.5, 0.5) on the CPU
    u8 = lambda *s: torch.randint(0, 256, s, device=dev, dtype=torch.uint8, generator=g)  # noqa: E731
    # ---- CQL_Offline
    n = 16
    mk = lambda: CQL_Offline(actor={"policy": {"num_layers": 3, "hidden_dim": 256}, "discrete_gripper": True},  # noqa: E731
                             critic={"q_network": {"num_layers": 3, "hidden_dim": 256, "last_layer_activation": "Identity"}},
                             real_world=True, obs_modalities=["rgb_static"], goal_modalities=["rgb_static"], action_dim=7,
                             device="cuda:0", compute_dtype="bf16", image_dtype="bf16", n_action_samples=4)
    o8, g8, x8 = u8(n, H, W, 3), u8(n, H, W, 3), u8(n, H, W, 3)
    act = torch.rand(n, 7, device=dev) * 2 - 1
    rew, done = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    chw = lambda x: tf(x).permute(0, 3, 1, 2).contiguous()  # noqa: E731
    mkb = lambda f: {"observations": {"observation": {"rgb_static": f(o8)}, "goal": {"rgb_static": f(g8)}}, "actions": act,  # noqa: E731
                     "next_observations": {"observation": {"rgb_static": f(x8)}, "goal": {"rgb_static": f(g8)}},
                     "rewards": rew, "terminals": done}
    b8, b32 = mkb(lambda x: x), mkb(chw)
    torch.manual_seed(0); ma = mk()
    torch.manual_seed(0); mb = mk()
    ma.training_step(b32, 0)
    mb.training_step(b8, 0)
    torch.cuda.synchronize()
    assert torch.equal(ma.engine.X3["rgb_static"], mb.engine.X3["rgb_static"])
    # ---- PlayLMP
    pr = dict(num_heads=8, num_layers=2, encoder_hidden_size=2048, fc_hidden_size=4096, latent_plan_dim=16, min_std=1e-4,
              dropout_p=0.0, max_position_embeddings=T)
    ad = dict(n_mixtures=10, num_layers=2, hidden_size=2048, out_features=7, num_classes=10, latent_plan_dim=16,
              rnn_model="rnn_decoder", include_goal=False)
    cams = ["rgb_static"]
    mkp = lambda: PlayLMP(plan_proposal={"policy": {"num_layers": 3, "hidden_dim": 256}}, plan_recognition=pr,  # noqa: E731
                          action_decoder=ad, plan_proposal_obs_modalities=cams, plan_proposal_goal_modalities=cams,
                          plan_recognition_modalities=cams, action_decoder_modalities=cams, real_world=True, device=dev,
                          compute_dtype="bf16", image_dtype="bf16")
    s8 = u8(8, T, H, W, 3)
    base = _batch(8)
    p32 = dict(base, states={"rgb_static": tf(s8).permute(0, 1, 4, 2, 3).contiguous()})
    p8 = dict(base, states={"rgb_static": s8})
    torch.manual_seed(0); pa = mkp()
    torch.manual_seed(0); pb = mkp()
    pa.training_step(p32, 0)
    pb.training_step(p8, 0)
    torch.cuda.synchronize()
    assert torch.equal(pa.frames["rgb_static"], pb.frames["rgb_static"])


@pytest.mark.parametrize("graph", [False, True])
def test_playlmp_branches_equal_serial(graph):
    """PlayLMP.training_step at bench shapes (bf16: ring GEMMs, fused encoder, one-launch RNN weight gradients) with its
    graph branches - random-plan decoder pass, plan-proposal backward, decoder weight gradients on side streams - and
    without: the same kernels on the same inputs, so logs and every gradient agree bit for bit (a race would show)."""
    import bench
    from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP

    dev = torch.device("cuda:0")
    B, T, cams = 64, 16, ["rgb_static"]
    actor = {"policy": {"num_layers": 3, "hidden_dim": 256}}
    pr = dict(num_heads=8, num_layers=2, encoder_hidden_size=2048, fc_hidden_size=4096, latent_plan_dim=16, min_std=1e-4,
              dropout_p=0.0, max_position_embeddings=T)
    ad = dict(n_mixtures=10, num_layers=2, hidden_size=2048, out_features=7, num_classes=10, latent_plan_dim=16,
              rnn_model="rnn_decoder", include_goal=False)
    batch = bench.synth_batch(B, T, 84, 84, dev, 1)
    res = []
    for branches in (True, False):
        torch.manual_seed(0)
        m = PlayLMP(plan_proposal=actor, plan_recognition=pr, action_decoder=ad, plan_proposal_obs_modalities=cams,
                    plan_proposal_goal_modalities=cams, plan_recognition_modalities=cams, action_decoder_modalities=cams,
                    real_world=True, device=dev, compute_dtype="bf16", image_dtype="bf16")
        m.branches = branches
        if graph:
            m.enable_graph()
        torch.manual_seed(5); torch.cuda.manual_seed(5)
        for _ in range(3):
            m.training_step(batch, 0)
        torch.cuda.synchronize()
        res.append((dict(m.logged), {k: v.clone() for k, v in m.named_gradients().items()},
                    {k: v.clone() for k, v in m.state_dict().items()}))
    (la, ga, pa), (lb, gb, pb) = res
    assert la == lb and all(v == v for v in la.values()), (la, lb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k


@pytest.mark.parametrize("B", [32, 64])
def test_playlmp_twin_pass_equals_own_pass(B):
    """PlayLMP.training_step (bf16, graph): the logging-only random-plan decoder pass as twin rows of the real pass's
    launches against a pass of its own - same weights, same inputs, the same per-element accumulation order in the ring
    GEMM: every log (random_plan_* included), every gradient and the stepped weights agree bit for bit."""
    import bench
    from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP

    dev = torch.device("cuda:0")
    T, cams = 16, ["rgb_static"]
    actor = {"policy": {"num_layers": 3, "hidden_dim": 256}}
    pr = dict(num_heads=8, num_layers=2, encoder_hidden_size=2048, fc_hidden_size=4096, latent_plan_dim=16, min_std=1e-4,
              dropout_p=0.0, max_position_embeddings=T)
    ad = dict(n_mixtures=10, num_layers=2, hidden_size=2048, out_features=7, num_classes=10, latent_plan_dim=16,
              rnn_model="rnn_decoder", include_goal=False)
    batch = bench.synth_batch(B, T, 84, 84, dev, 1)
    res = []
    for twin in (True, False):
        torch.manual_seed(0)
        m = PlayLMP(plan_proposal=actor, plan_recognition=pr, action_decoder=ad, plan_proposal_obs_modalities=cams,
                    plan_proposal_goal_modalities=cams, plan_recognition_modalities=cams, action_decoder_modalities=cams,
                    real_world=True, device=dev, compute_dtype="bf16", image_dtype="bf16")
        m.ad.twin_pass = twin
        assert bool(m.ad.twin_ok(B, m.compute)) == twin
        m.enable_graph()
        torch.manual_seed(5); torch.cuda.manual_seed(5)
        for _ in range(3):
            m.training_step(batch, 0)
        torch.cuda.synchronize()
        res.append((dict(m.logged), {k: v.clone() for k, v in m.named_gradients().items()},
                    {k: v.clone() for k, v in m.state_dict().items()}))
    (la, ga, pa), (lb, gb, pb) = res
    assert la == lb and all(v == v for v in la.values()), (la, lb)
    assert any("random_plan_action_loss" in k for k in la)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k


def test_bptt_wavefront_equals_per_layer():
    """Action-decoder backward at bench shapes: the wavefront of batched ring-GEMM launches (both layers' recurrent
    gradient steps + the projection onto the lower layer per launch) against one launch per (layer, step) + a projection
    GEMM: same products in the same K order - the gradients agree to fp32 rounding; and the square weight gradients behind the
    wavefront as one launch against one launch per matrix: bit-identical."""
    import bench
    from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP

    dev = torch.device("cuda:0")
    B, T, cams = 128, 16, ["rgb_static"]
    actor = {"policy": {"num_layers": 3, "hidden_dim": 256}}
    pr = dict(num_heads=8, num_layers=2, encoder_hidden_size=2048, fc_hidden_size=4096, latent_plan_dim=16, min_std=1e-4,
              dropout_p=0.0, max_position_embeddings=T)
    ad = dict(n_mixtures=10, num_layers=2, hidden_size=2048, out_features=7, num_classes=10, latent_plan_dim=16,
              rnn_model="rnn_decoder", include_goal=False)
    batch = bench.synth_batch(B, T, 84, 84, dev, 1)
    res = []
    for wavefront, batched in ((True, True), (False, True), (True, False)):
        torch.manual_seed(0)
        m = PlayLMP(plan_proposal=actor, plan_recognition=pr, action_decoder=ad, plan_proposal_obs_modalities=cams,
                    plan_proposal_goal_modalities=cams, plan_recognition_modalities=cams, action_decoder_modalities=cams,
                    real_world=True, device=dev, compute_dtype="bf16", image_dtype="bf16")
        m.ad.bptt_wavefront, m.ad.wgrad_batched = wavefront, batched
        torch.manual_seed(5); torch.cuda.manual_seed(5)
        m.training_step(batch, 0)
        torch.cuda.synchronize()
        res.append((dict(m.logged), {k: v.clone() for k, v in m.named_gradients().items()}))
    (la, ga), (lb, gb), (_, gc) = res
    for k in ga:  # the square weight gradients as one launch (tacorl_rnn_wgrad_batch) or one launch each: the same sums
        assert torch.equal(ga[k], gc[k]), k
    assert all(v == v for v in la.values())
    for k in la:
        assert abs(la[k] - lb[k]) <= 1e-6 * max(1.0, abs(lb[k])), (k, la[k], lb[k])
    for k in ga:
        d = (ga[k] - gb[k]).norm() / gb[k].norm().clamp_min(1e-30)
        assert d < 2e-5, (k, d.item())


# ---------------------------------------------------------------------------------------------------------------------
# BASELINE configs[2] (C3: the default TACORL step, action-decoder fine-tuning on, B=256), configs[3] (C4: one GPU's share
# of the dual-camera 128x128 real-world batch - 512 / 8 = 64 samples, window 32, latent 32) and configs[0] (C1: PlayLMP,
# B=32) at FULL size against the oracle: exact-fp32 mode at the north-star 1e-4, bf16 mode against the oracle evaluated
# with the MFMA's operand rounding.  (tests/test_step_gpu.py holds the same configurations at fixture size against the
# reference's own outputs; the 128x128 row-band encoder, the two-band conv1 weight gradient and the large-row MLP /
# RNN instantiations only run at these sizes.)
def _build_tacorl(compute, cams, T, latent, finetune):
    from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP
    from tacorl_amd.modules.tacorl.tacorl import TACORL

    names = sorted(cams)
    actor = {"policy": {"num_layers": 3, "hidden_dim": 256}}
    critic = {"q_network": {"num_layers": 3, "hidden_dim": 256, "last_layer_activation": "Identity"}}
    pr = dict(num_heads=8, num_layers=2, encoder_hidden_size=2048, fc_hidden_size=4096, latent_plan_dim=latent,
              min_std=1e-4, dropout_p=0.0, max_position_embeddings=T)
    ad = dict(n_mixtures=10, num_layers=2, hidden_size=2048, out_features=7, num_classes=10, latent_plan_dim=latent,
              rnn_model="rnn_decoder", include_goal=False)
    torch.manual_seed(3)
    lmp = PlayLMP(plan_proposal=actor, plan_recognition=pr, action_decoder=ad, plan_proposal_obs_modalities=names,
                  plan_proposal_goal_modalities=names, plan_recognition_modalities=names, action_decoder_modalities=names,
                  real_world=True, device="cuda:0", compute_dtype=compute, image_dtype=compute)
    mod = TACORL(play_lmp=lmp, finetune_action_decoder=finetune, critic=critic, real_world=True, device="cuda:0",
                 compute_dtype=compute, image_dtype=compute, action_decoder_lr=3e-4, actor_lr=1e-4, critic_lr=3e-4,
                 discount=0.95, conservative_weight=1.0, reward_scale=10.0, n_action_samples=4, with_lagrange=True,
                 deterministic_backup=True, bc_epochs=5)
    mod.current_epoch = 5
    return mod


def _tacorl_oracle(mod, cams, latent, finetune):
    from oracle import tacorl_oracle as O

    names = sorted(cams)
    spec = O.ACSpec(cams=names, goal_cams=names, action_dim=latent, n=4, discount=0.95, actor_lr=1e-4, critic_lr=3e-4,
                    deterministic_backup=True, reward_scale=10.0, bc_epochs=5, with_lagrange=True, discrete_gripper=False,
                    target_entropy=-7.0, finetune_action_decoder=finetune, ac_cams=names, pr_cams=names,
                    action_decoder_lr=3e-4)
    skip = ("one_hot_embedding_eye", "ones", "gripper_bounds", "action_max_bound", "action_min_bound")
    P = {k: v.detach().cpu().clone().contiguous() for k, v in mod.state_dict().items()
         if v.dtype == torch.float32 and not any(k.endswith(s) for s in skip)}
    frozen = ("perceptual_encoder.", "plan_recognition.") + (() if finetune else ("action_decoder.",))
    O.require_grad_(P, frozen_prefixes=frozen)
    return O, spec, P


def _compare(got, ologs, rtol, grads=None, ograds=None, grad_rtol=None, plan=None, oplan=None, min_common=8, acc_atol=None):
    """acc_atol: absolute tolerance for the *_accuracy logs - means of 0/1 argmax decisions, which move in steps of 1 / rows when
    a near-tie flips under another operand rounding (bf16 comparisons only: a few decisions)."""
    bad = []
    common = set(ologs) & set(got)
    assert len(common) >= min_common, (sorted(ologs), sorted(got))
    for k in sorted(common):
        v = float(ologs[k])
        if acc_atol is not None and k.endswith("accuracy"):
            if abs(got[k] - v) > acc_atol:
                bad.append(f"{k}: hip {got[k]:.8g} oracle {v:.8g} (more than {acc_atol:.4g} apart)")
            continue
        if abs(got[k] - v) > rtol * max(abs(v), 1e-3):
            bad.append(f"{k}: hip {got[k]:.8g} oracle {v:.8g}")
    if plan is not None:
        e = ((plan.cpu() - oplan).norm() / oplan.norm()).item()
        if e > rtol:
            bad.append(f"latent plan relerr {e:.3g}")
    if grads is not None:
        top = max(g.norm().item() for g in ograds.values() if g is not None)
        for k, g in ograds.items():
            if k in grads and g is not None and g.norm() > 1e-6 * top:
                d = ((grads[k].cpu().reshape(g.shape) - g).norm() / g.norm()).item()
                if d > grad_rtol:
                    bad.append(f"grad {k}: relerr {d:.3g}")
    return bad


FULL_TACORL = {
    # name: (B, T, cameras, latent, fine-tune the action decoder)
    "c2": (256, 16, {"rgb_static": (84, 84)}, 16, False),  # the headline configuration (BASELINE configs[1])
    "c3": (256, 16, {"rgb_static": (84, 84)}, 16, True),
    "c4_share": (64, 32, {"rgb_static": (128, 128), "rgb_gripper": (128, 128)}, 32, False),
    # experiment=tacorl_real_world at the reference's own geometry (rgb_static un-resized, rl_real_world_train.yaml:2-10): in bf16
    # every problem of the 150 x 200 camera takes encoder_ring.hip's fused forward, the ones a backward follows also the
    # LDS-resident backward (tests/test_encoder_stage_cpu.py pins that plan: case ac_ring)
    "c4_real": (16, 32, {"rgb_static": (150, 200), "rgb_gripper": (84, 84)}, 32, False),
}


@pytest.mark.parametrize("name", sorted(FULL_TACORL))
def test_fullsize_tacorl_configs_f32_match_oracle(name):
    from tacorl_amd import synth

    Bn, Tn, cams, latent, finetune = FULL_TACORL[name]
    mod = _build_tacorl("f32", cams, Tn, latent, finetune)
    O, spec, P = _tacorl_oracle(mod, cams, latent, finetune)
    opts = O.make_opts(P, spec)
    batch = synth.make_play_batch(4200 + len(name), Bn, Tn, cams)
    mod.logged = {}
    mod.training_step(_to_dev(batch, mod.device))
    got, nz = _logs(mod), _cpu(_noise(mod))
    ologs, oplan, ograds = O.tacorl_step(P, opts, spec, batch, nz, 5)
    bad = _compare(got, ologs, 1e-4, mod.named_gradients(), ograds, 1e-3, mod.plan, oplan)
    if finetune:
        assert "action_loss" in got and any(k.startswith("action_decoder.") for k in ograds)
    assert not bad, "\n".join(bad[:30])


def _bf16_grad_check(mod, eval_rounded, eval_f32, P_before, ograds):
    """Full-size bf16 gradients against the rounded oracle, norm-wise per tensor: tolerance max(1e-2, 3 x the tensor's
    reproducibility floor) - the floor is how far the rounded oracle's own gradient moves under a 1-ulp perturbation of
    the parameters (golden_util.gradient_floor, 2 runs) or a sixth of what bf16 rounding changes at all
    (test_step_gpu._with_bf16_sensitivity) - every comparison recorded through record_margin.
    eval_*(P) -> {name: gradient} must not modify P's originals."""
    from oracle import tacorl_oracle as O
    from tests.golden_util import gradient_floor
    from tests.test_step_gpu import _snap, _with_bf16_sensitivity, compare_with_oracle_grads

    with O.operand_rounding(torch.bfloat16):
        floor = gradient_floor(eval_rounded, P_before, ograds, runs=2)
    floor = _with_bf16_sensitivity(floor, ograds, eval_f32(_snap(P_before)))
    return compare_with_oracle_grads(mod, ograds, 1e-2, floor)


@pytest.mark.parametrize("name", sorted(FULL_TACORL))
def test_fullsize_tacorl_configs_bf16_vs_rounded_oracle(name):
    """The benchmarked mode at full size (C2 = the headline step, C3, C4's share): losses and plans against the oracle
    evaluated with bf16 operand rounding in every contraction (2e-3 relative: what is left is accumulation order), and
    every gradient norm-wise against the same oracle (1e-2 or 3 x its reproducibility floor)."""
    import copy

    from tacorl_amd import synth
    from tests.test_step_gpu import _snap

    Bn, Tn, cams, latent, finetune = FULL_TACORL[name]
    mod = _build_tacorl("bf16", cams, Tn, latent, finetune)
    O, spec, P = _tacorl_oracle(mod, cams, latent, finetune)
    opts = O.make_opts(P, spec)
    batch = synth.make_play_batch(4300 + len(name), Bn, Tn, cams)
    mod.logged = {}
    mod.training_step(_to_dev(batch, mod.device))
    got, nz = _logs(mod), _cpu(_noise(mod))
    before, opts0 = _snap(P), copy.deepcopy(opts)
    with O.operand_rounding(torch.bfloat16):
        ologs, oplan, ograds = O.tacorl_step(P, opts, spec, batch, nz, 5)
    bad = _compare(got, ologs, 2e-3, plan=mod.plan, oplan=oplan)
    ev = lambda Pp: O.tacorl_step(Pp, copy.deepcopy(opts0), spec, batch, nz, 5)[2]  # noqa: E731
    bad += _bf16_grad_check(mod, ev, ev, before, ograds)
    if finetune:  # (the decoder's BPTT / weight-gradient kernels on the step's own inputs and head gradients)
        cam = mod.action_decoder_modalities[0]
        bad += _decoder_backward_in_situ(mod, before, f"{name} bf16", mod.ad, mod.plan, mod.f_out[cam], Bn, Tn)
    assert not bad, "\n".join(bad[:30])


def test_fullsize_cql_baseline_c5_bf16_vs_rounded_oracle():
    """BASELINE configs C5 at its stated size (B=1024, n=32: the Q networks run over 99 328 rows - the many-row MLP
    kernels) in the benchmarked bf16 mode against the oracle with bf16 operand rounding: every logged loss 2e-3, every
    gradient norm-wise 1e-2 (or 3 x floor)."""
    import copy

    from oracle import tacorl_oracle as O
    from tacorl_amd import synth
    from tacorl_amd.init import init_views_
    from tacorl_amd.modules.cql.cql_offline_lightning import CQL_Offline
    from tests.test_step_gpu import _snap

    dev = torch.device("cuda:0")
    Bc, n = 1024, 32
    torch.manual_seed(3)
    mod = CQL_Offline(actor={"policy": {"num_layers": 3, "hidden_dim": 256}, "discrete_gripper": True},
                      critic={"q_network": {"num_layers": 3, "hidden_dim": 256, "last_layer_activation": "Identity"}},
                      real_world=True, obs_modalities=["rgb_static"], goal_modalities=["rgb_static"], action_dim=7, device="cuda:0",
                      compute_dtype="bf16", image_dtype="bf16", discount=0.99, actor_lr=1e-4, critic_lr=3e-4,
                      conservative_weight=1.0, n_action_samples=n, with_lagrange=True, reward_scale=10.0,
                      deterministic_backup=False, bc_epochs=5)
    mod.current_epoch = 5
    for blk in (mod.engine.actor, mod.engine.q1, mod.engine.q2):
        init_views_(blk.views)
    mod.sync_targets()
    cams = ["rgb_static"]
    spec = O.ACSpec(cams=cams, goal_cams=cams, action_dim=7, n=n, discount=0.99, actor_lr=1e-4, critic_lr=3e-4,
                    deterministic_backup=False, reward_scale=10.0, bc_epochs=5, with_lagrange=True,
                    discrete_gripper=True, target_entropy=-7.0)
    P = {k: v.detach().cpu().clone().contiguous() for k, v in mod.state_dict().items()}
    O.require_grad_(P)
    opts = O.make_opts(P, spec)
    batch = synth.make_transition_batch(7, Bc, {"rgb_static": (84, 84)})
    mod.logged = {}
    mod.training_step(_to_dev(batch, dev), 0)
    torch.cuda.synchronize()
    got = {k.split("/", 1)[1]: float(v) for k, v in mod.logged.items()}
    nz = {k: v.detach().cpu().clone() for k, v in mod.engine.noise.items()}
    before, opts0 = _snap(P), copy.deepcopy(opts)
    with O.operand_rounding(torch.bfloat16):
        ologs, ograds = O.cql_step(P, opts, spec, batch, nz, 5)
    # (Q heads start at +-1e-3: q*_data / random / policy are ~1e-2 sums, hence the 5e-2 floor of the relative scale -
    # as in tests/test_step_gpu.py::_bf16_compare)
    bad = [f"{k}: hip {got[k]:.8g} rounded oracle {float(v):.8g}" for k, v in ologs.items()
           if k in got and abs(got[k] - float(v)) > 2e-3 * max(abs(float(v)), 5e-2)]
    assert len(set(ologs) & set(got)) >= 8, (sorted(ologs), sorted(got))
    ev = lambda Pp: O.cql_step(Pp, copy.deepcopy(opts0), spec, batch, nz, 5)[1]  # noqa: E731
    bad += _bf16_grad_check(mod, ev, ev, before, ograds)
    assert not bad, "\n".join(bad[:30])


def _encoder_backward_in_situ(mod, P, batch, ograds):
    """VERDICT r4 #6.  PlayLMP's encoder gradients sit 3-5 % (convolutions) and 20-30 % (soft-argmax temperature) from the
    rounded oracle in bf16 mode, and the bisect (profiles/r05_playlmp_bf16_bisect.md, scratch/r5_bisect_plmp.py) says
    where that comes from: the gradient that ENTERS the encoder's backward, d_emb, moves by 7 % under bf16 rounding of the
    decoder's recurrent network alone (30 sequential layers of BPTT) and by 4 % under a 1e-7 perturbation of the
    parameters; the temperature gradient - one global (dp - <p, dp>) cancellation - amplifies it threefold.  None of that
    is the encoder backward's own error.  This check removes the upstream: the step's OWN d_emb (read back from the
    module) is pushed through the oracle's encoder backward under bf16 operand rounding, and the HIP conv / FC / temperature
    gradients of the same step are held to THAT - tolerances 1.5e-2 (weights and biases) and 5e-2 (temperature), nothing
    widened.  The d_emb error against the rounded oracle's own d_emb is recorded beside it."""
    from oracle import tacorl_oracle as O
    from tests.golden_util import record_margin

    cam = "rgb_static"
    pre = f"perceptual_encoder.networks.{cam}."
    st = batch["states"][cam]
    B, T = st.shape[:2]
    Pe = {k: v.detach().clone().requires_grad_(True) for k, v in P.items() if k.startswith(pre)}
    d_emb = mod.d_emb.detach().cpu().reshape(B * T, -1)[:, :32].contiguous()
    with O.operand_rounding(torch.bfloat16):
        emb = O.encoder_fwd(Pe, pre, st.reshape(B * T, *st.shape[2:]))
        names = sorted(Pe)
        gs = torch.autograd.grad(emb, [Pe[n] for n in names], grad_outputs=d_emb)
        ex = {}
        O.playlmp_step({k: v.detach().clone().requires_grad_(True) for k, v in P.items()}, None, batch,
                       {k: v for k, v in _last_noise.items()}, [cam], step=False, extra=ex)
    e_up = ((d_emb - ex["d_emb"].reshape(B * T, -1)).norm() / ex["d_emb"].norm()).item()
    record_margin("C1 bf16: d_emb entering the encoder backward (HIP vs rounded oracle)", e_up, float("nan"), kind="upstream of the encoder backward")
    got = mod.named_gradients()
    bad = []
    for n, gexp in zip(names, gs):
        tol = 5e-2 if n.endswith("temperature") else 1.5e-2
        e = ((got[n].detach().cpu().reshape(gexp.shape) - gexp).norm() / gexp.norm().clamp_min(1e-30)).item()
        e_full = ((got[n].detach().cpu().reshape(gexp.shape) - ograds[n]).norm() / ograds[n].norm().clamp_min(1e-30)).item()
        record_margin(f"C1 bf16 in situ (own d_emb): {n}", e, tol, kind=f"encoder backward vs rounded oracle; vs the whole-step oracle {e_full:.3g}")
        if e > tol:
            bad.append(f"in-situ encoder backward {n}: relerr {e:.3g} (tolerance {tol:.3g}; against the whole-step oracle {e_full:.3g}, d_emb off by {e_up:.3g})")
    return bad


def _decoder_backward_in_situ(mod, P, label, ad, plan, emb, B, T, pre="action_decoder."):
    """the tight row for the ring-GEMM BPTT / RNN weight-gradient kernels, as `_encoder_backward_in_situ` is
    for the conv backward.  End to end the decoder's gradients can only be held to the oracle's own reproducibility (30
    sequential ReLU layers amplify one flipped bf16 rounding: floors of 1 - 8 %).  Here the upstream is removed: the
    step's OWN inputs (plan, frame embeddings) and its OWN dL/d(heads) - read back from the module - go through the
    oracle's decoder forward and autograd under bf16 operand rounding, and the HIP gradients of every decoder parameter
    (rnn.weight_ih / weight_hh / bias_* of both layers, the four heads) are held to that at 1.5e-2, nothing widened."""
    from oracle import tacorl_oracle as O
    from tests.golden_util import record_margin

    Tm = T - 1
    names = sorted(k for k in P if k.startswith(pre))
    Pd = {k: P[k].detach().clone().requires_grad_(True) for k in names}
    L = sum(1 for k in names if "rnn.weight_hh_l" in k)
    pl = plan.detach().cpu().float()
    em = emb.detach().cpu().float().reshape(B, T, -1)[:, :Tm]
    NH = Pd[pre + "mean_fc.weight"].shape[0] * 3 + 2
    # module rows are time-major (row t * B + b), the head columns [mean | log_scale | prob | gripper]
    dh = ad.d_heads.detach().cpu()[: Tm * B, :NH].reshape(Tm, B, NH).transpose(0, 1).contiguous()
    with O.operand_rounding(torch.bfloat16):
        x = torch.cat([pl.unsqueeze(1).expand(-1, Tm, -1), em], dim=-1)
        O._REGION.append("rnn")
        for l in range(L):
            wi, wh = Pd[f"{pre}rnn.weight_ih_l{l}"], Pd[f"{pre}rnn.weight_hh_l{l}"]
            bi, bh = Pd[f"{pre}rnn.bias_ih_l{l}"], Pd[f"{pre}rnn.bias_hh_l{l}"]
            h = torch.zeros(B, wh.shape[0])
            xin = O._linear(x, wi, bi)
            outs = []
            for t in range(Tm):
                h = torch.relu(xin[:, t] + O._linear(h, wh, bh))
                outs.append(h)
            x = torch.stack(outs, dim=1)
        heads = torch.cat([O._linear(x, Pd[pre + f"{n}.weight"], Pd[pre + f"{n}.bias"])
                           for n in ("mean_fc", "log_scale_fc", "prob_fc", "gripper_fc")], dim=-1)
        O._REGION.pop()
        gs = torch.autograd.grad(heads, [Pd[n] for n in names], grad_outputs=dh)
    got = mod.named_gradients()
    bad = []
    for n, gexp in zip(names, gs):
        if n not in got or gexp.norm() == 0:
            continue
        tol = 1.5e-2
        e = ((got[n].detach().cpu().reshape(gexp.shape) - gexp).norm() / gexp.norm().clamp_min(1e-30)).item()
        record_margin(f"{label} in situ (own plan, embeddings, d_heads): {n}", e, tol, kind="decoder BPTT + weight gradients vs rounded oracle")
        if e > tol:
            bad.append(f"in-situ decoder backward {n}: relerr {e:.3g} (tolerance {tol:.3g})")
    return bad


_last_noise = {}


@pytest.mark.parametrize("compute,rtol", [("f32", 1e-4), ("bf16", 2e-3)])
def test_fullsize_playlmp_c1_matches_oracle(compute, rtol):
    """BASELINE configs[0]: PlayLMP.training_step at batch 32 (84x84, window 16)."""
    from oracle import tacorl_oracle as O
    from tacorl_amd import synth
    from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP
    from tests import cfg_util as C

    cams = {"rgb_static": (84, 84)}
    strip = lambda c: {k: v for k, v in c.items() if k not in ("_target_", "_recursive_")}  # noqa: E731
    torch.manual_seed(4)
    mod = PlayLMP(**strip(C.playlmp_cfg(device="cuda:0", compute_dtype=compute, image_dtype=compute)))
    P = {k: v.detach().cpu().clone().contiguous() for k, v in mod.state_dict().items() if v.dtype == torch.float32}
    P = {k: v for k, v in P.items() if k in dict(mod.named_parameters())}
    O.require_grad_(P)
    opt = O.Adam([n for n in P], 1e-4)
    batch = synth.make_play_batch(4400, 32, 16, cams)
    mod.logged = {}
    mod.training_step(_to_dev(batch, mod.device), 0)
    torch.cuda.synchronize()
    got = {k.split("/", 1)[1]: float(v) for k, v in mod.logged.items()}
    nz = {k: v.cpu().clone() for k, v in mod.noise.items()}
    g = torch.Generator().manual_seed(9)
    nz["rand"] = [torch.rand(32, 15, 6, 10, generator=g), torch.rand(32, 15, 6, generator=g),
                  torch.rand(32, 15, 6, 10, generator=g), torch.rand(32, 15, 6, generator=g)]
    nz["u_goal"] = torch.rand(32, 32, generator=g)
    _last_noise.clear()
    _last_noise.update(nz)
    if compute == "bf16":
        with O.operand_rounding(torch.bfloat16):
            ologs, ograds = O.playlmp_step(P, opt, batch, nz, ["rgb_static"], step=False)
        bad = _compare(got, ologs, rtol, min_common=5, acc_atol=3.0 / (32 * 15))  # (3 of the 480 gripper decisions)
        ev = lambda Pp: O.playlmp_step(Pp, opt, batch, nz, ["rgb_static"], step=False)[1]  # noqa: E731
        bad += _bf16_grad_check(mod, ev, ev, P, ograds)
        bad += _encoder_backward_in_situ(mod, P, batch, ograds)
        bad += _decoder_backward_in_situ(mod, P, "C1 bf16", mod.ad, mod.plan, mod.emb, 32, 16)
    else:
        ologs, ograds = O.playlmp_step(P, opt, batch, nz, ["rgb_static"], step=False)
        bad = _compare(got, ologs, rtol, mod.named_gradients(), ograds, 1e-3, min_common=5)
    assert not bad, "\n".join(bad[:30])


def test_bf16_graph_replay_sees_in_place_parameter_edits():
    """a replayed bf16 step reads weight-derived copies (the fused encoder's packed conv fragments, packed behind
    the previous step's Adam launch; bf16 mirrors of the MLP weights) whose freshness is tracked through torch version
    counters.  Replay, edit parameters in place the ways a user can (a conv weight and an MLP weight through their
    nn.Parameter views, load_state_dict of a perturbed copy), replay again: the graph module must end bit-identical to an
    eager twin that saw the same edits - and an undisturbed run must not re-capture."""
    batch = _batch(64)
    mods = {g: _mod("bf16", g) for g in (True, False)}
    captures = []
    orig = type(mods[True])._capture_only

    def counting(self, *a, **k):
        captures.append(1)
        return orig(self, *a, **k)

    for m in mods.values():
        m._capture_only = counting.__get__(m)
    ends = {}
    for g, m in mods.items():
        torch.manual_seed(5)
        for _ in range(4):
            m.training_step(batch)
        if g:
            assert len(captures) == 1, "an undisturbed run replays its one capture"
        sd = m.state_dict()
        conv = next(k for k in sd if k.startswith("q1.") and k.endswith("model.0.weight"))
        lin = next(k for k in sd if k.startswith("actor.") and "fc_layers.0.weight" in k)
        with torch.no_grad():
            dict(m.named_parameters())[conv].mul_(1.03)
            dict(m.named_parameters())[lin].add_(0.01)
        for _ in range(2):
            m.training_step(batch)
        pert = {k: (v * 0.99 if v.dtype == torch.float32 and k.startswith("q2.") else v) for k, v in m.state_dict().items()}
        m.load_state_dict(pert)
        for _ in range(2):
            m.training_step(batch)
        torch.cuda.synchronize()
        ends[g] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    diff = [k for k in ends[True] if not torch.equal(ends[True][k], ends[False][k])]
    assert not diff, diff[:10]
