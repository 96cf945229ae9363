"""The vector-observation (D4RL) modules on the GPU: play_lmp_d4rl.PlayLMP and tacorl_d4rl.TACORL replay the noise of the goldens
tools/gen_d4rl_golden.py recorded from the unmodified reference, two free-running steps each, f32 at the project's parity bar
(1e-4 relative on every logged loss, on the sampled plans and on the parameter fingerprints; gradients at the image tests'
GRAD_RTOL against the restatement tests/d4rl_ref.py on the module's own parameters and against the golden fingerprints), with
the step captured as ONE graph: the first call runs eagerly and captures, the second is a replay.  Validation moves nothing.
bf16 is held to the restatement evaluated with the MFMA's operand rounding by the helper and margins of the image modules'
bf16 tests (tests/test_step_gpu.py: the dense arithmetic is the same kernels).  Two ranks on per-sample shards equal one rank
on the full batch at B = 4 (tests/d4rl_shard_script.py, the mechanism of tests/test_dist_gpu.py)."""
import copy
import os
import sys

import pytest
import torch

from tests import d4rl_cfg as K
from tests import d4rl_ref as R
from tests.golden_util import check_stats, gradient_floor, resync_oracle
from tests.proc_util import free_port, run_group
from tests.test_step_gpu import (GRAD_RTOL, PARAM_ATOL, RTOL, L_as_list, _bf16_compare, _snap, _with_bf16_sensitivity, check_logs,
                                 compare_with_oracle_grads, relerr, to_dev)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def build_playlmp(g, compute="f32", **over):
    return K.build(K.playlmp_d4rl_cfg(latent=g.cfg["latent"], T=g.cfg["T"], device=DEV, compute_dtype=compute,
                                      dropout_p=g.cfg.get("dropout_p", 0.0), **over))


def build_tacorl(g, compute="f32", **over):
    lmp = build_playlmp(g, compute)
    return K.build(K.tacorl_d4rl_cfg(play_lmp=lmp, finetune_action_decoder=g.cfg["finetune_ad"], device=DEV,
                                     compute_dtype=compute, **over))


def _logged(mod):
    return {k.split("/", 1)[1]: v for k, v in mod.logged.items()}


def _grads_vs_restatement(mod, ograds, floor_fn):
    """GRAD_RTOL; a tensor that misses it is held to three times its own reproducibility under a 1-ulp perturbation of the
    parameters (golden_util.gradient_floor, as tests/test_step_gpu.py does) - evaluated only when something misses."""
    bad = compare_with_oracle_grads(mod, ograds, GRAD_RTOL)
    return compare_with_oracle_grads(mod, ograds, GRAD_RTOL, floor_fn()) if bad else bad


def _same_graph(mod, seen):
    """One captured graph for the step; `seen`: the graph objects of the previous call - a replay leaves them as they are."""
    assert len(mod._graphs) == 1
    gs, g_side, _ = next(iter(mod._graphs.values()))
    assert len(gs) == 1 and g_side is None
    if seen is not None:
        assert seen is gs, "the step was captured again instead of replayed"
    return gs


@pytest.mark.parametrize("name", ["tacorl_d4rl_q", "tacorl_d4rl_ad"])
def test_tacorl_d4rl_step(name):
    from oracle import tacorl_oracle as O

    g = K.D4rlGolden(name)
    mod = build_tacorl(g)
    assert {n: list(p.shape) for n, p in mod.named_parameters()} == dict(zip(g.names, g.shapes))
    missing, unexpected = mod.load_state_dict(g.params(), strict=False)
    assert not unexpected and all(m.startswith("action_decoder.") and "weight" not in m and "bias" not in m for m in missing)
    mod.enable_graph()
    spec = R.Spec(finetune_action_decoder=g.cfg["finetune_ad"])
    P = R.require_grad_(g.params())
    opts = O.make_opts(P, spec)
    seen = None
    for step in range(g.cfg["steps"]):
        batch, noise = g.batch(step), g.noise(step)
        if step:
            resync_oracle(mod, P, opts)  # gradients of step > 0: against the restatement on the module's own parameters
        mod.logged = {}
        mod.training_step(to_dev(batch, mod.device), noise=to_dev(noise, mod.device))
        torch.cuda.synchronize()
        seen = _same_graph(mod, seen)
        got = _logged(mod)
        before, opts0 = _snap(P), copy.deepcopy(opts)
        _, oplan, ograds = R.tacorl_step(P, opts, spec, batch, noise, 0)
        exp = g.logged(step)
        assert set(exp) == set(got), (sorted(set(exp) ^ set(got)))
        bad = check_logs(got, exp)
        e = relerr(mod.engine.action, g.latent_plan(step))
        if e > RTOL:
            bad.append(f"latent plan relerr {e:.3g} (restatement {relerr(mod.engine.action, oplan):.3g})")
        bad += _grads_vs_restatement(mod, ograds, lambda: gradient_floor(
            lambda Pp: R.tacorl_step(Pp, copy.deepcopy(opts0), spec, batch, noise, 0)[2], before, ograds))
        assert set(ograds) <= set(mod.named_gradients())
        if step == 0:  # (fingerprints of later steps' gradients belong to the reference's own parameter trajectory)
            bad += check_stats(mod.named_gradients(), g.stats(step, "grad"), rtol=GRAD_RTOL, what="golden grad ")
        bad += check_stats(mod.state_dict(), g.stats(step, "param"), rtol=RTOL, atol=PARAM_ATOL, what="golden param ")
        assert not bad, f"step {step}:\n" + "\n".join(bad[:25])


def test_playlmp_d4rl_step():
    from oracle import tacorl_oracle as O

    g = K.D4rlGolden("playlmp_d4rl")
    mod = build_playlmp(g)
    assert {n: list(p.shape) for n, p in mod.named_parameters()} == dict(zip(g.names, g.shapes))
    mod.load_state_dict(g.params(), strict=False)
    mod.enable_graph()
    P = O.require_grad_(g.params())
    opt = O.Adam([n for n in P], 1e-4)
    dp, seen = g.cfg["dropout_p"], None
    for step in range(g.cfg["steps"]):
        batch, nz = g.batch(step), g.noise(step)
        assert len(nz["dropout"]) == 9  # the embedding mask + four per encoder layer
        if step:
            resync_oracle(mod, P, opt)
        mod.logged = {}
        total = mod.training_step(to_dev(batch, mod.device), 0, noise=nz)
        torch.cuda.synchronize()
        seen = _same_graph(mod, seen)
        got = _logged(mod)
        before, opt0 = _snap(P), copy.deepcopy(opt)
        _, ograds, oplan = R.playlmp_step(P, opt, batch, nz, dropout_p=dp)
        exp = g.logged(step)
        assert set(exp) == set(got), sorted(set(exp) ^ set(got))
        bad = check_logs(got, exp)
        if abs(total - exp["total_loss"]) > RTOL * abs(exp["total_loss"]):
            bad.append(f"returned total {total!r} vs {exp['total_loss']!r}")
        e = relerr(mod.plan, oplan)
        if e > RTOL:
            bad.append(f"sampled plan relerr {e:.3g}")
        bad += _grads_vs_restatement(mod, ograds, lambda: gradient_floor(
            lambda Pp: R.playlmp_step(Pp, copy.deepcopy(opt0), batch, nz, dropout_p=dp)[1], before, ograds))
        if step == 0:
            bad += check_stats(mod.named_gradients(), g.stats(step, "grad"), rtol=GRAD_RTOL, what="golden grad ")
        bad += check_stats(mod.state_dict(), g.stats(step, "param"), rtol=RTOL, atol=PARAM_ATOL if step == 0 else 2e-4,
                           what="golden param ")
        assert not bad, f"step {step}:\n" + "\n".join(bad[:25])


def test_tacorl_d4rl_validation_step():
    """Every `validation/*` scalar of the golden, the sampled plan, and nothing moves: parameters, targets, Adam state."""
    g = K.D4rlGolden("val_tacorl_d4rl")
    mod = build_tacorl(g)
    mod.load_state_dict(g.params(), strict=False)
    mod.eval()
    before = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    opt_before = [o.state_dict() for o in L_as_list(mod.configure_optimizers())]
    mod.logged = {}
    mod.validation_step(to_dev(g.batch(0), mod.device), 0, noise=to_dev(g.noise(0), mod.device))
    torch.cuda.synchronize()
    assert mod.logged and all(k.startswith("validation/") for k in mod.logged), sorted(mod.logged)
    got, exp = _logged(mod), g.logged(0)
    assert set(exp) == set(got), sorted(set(exp) ^ set(got))
    bad = check_logs(got, exp)
    err = relerr(mod.engine.action, g.latent_plan(0))
    if err > RTOL:
        bad.append(f"latent plan relerr {err:.3g}")
    after = mod.state_dict()
    bad += [f"{k} moved" for k, v in before.items() if not torch.equal(v, after[k])]
    for o0, o in zip(opt_before, L_as_list(mod.configure_optimizers())):
        s1 = o.state_dict()["state"]
        for i, st in o0["state"].items():
            if not all(torch.equal(st[f], s1[i][f]) for f in ("step", "exp_avg", "exp_avg_sq")):
                bad.append(f"optimizer {o.name}: state of parameter {i} moved")
    assert not bad, "\n".join(bad[:25])


def test_cql_offline_d4rl_step():
    """The flat baseline TACORL-D4RL derives from (no golden: the reference's D4RL experiments train TACORL): one f32 step on
    transition rows `[state | goal]` against the restatement's update with the same injected noise - logged scalars at 1e-4,
    every gradient at GRAD_RTOL, the parameters after the step."""
    from oracle import tacorl_oracle as O
    from tacorl_amd import synth

    B, n, A, S = 3, 4, K.ACTION_DIM, K.STATE_DIM + K.GOAL_DIM
    mod = K.build(K.cql_d4rl_cfg(device=DEV))
    names = {k: list(v.shape) for k, v in mod.named_parameters()}
    params = {k: synth.param_values(k, s, 71) for k, s in names.items()}
    mod.load_state_dict(params)
    gen = torch.Generator().manual_seed(72)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    reward = torch.tensor([1, 0, 0])
    batch = dict(observations=r(B, S), next_observations=r(B, S), actions=torch.tanh(r(B, A)), rewards=reward, terminals=reward.clone())
    noise = dict(eps_pi=r(B, A), eps_next=r(B, A), u_rand=torch.rand(n * B, A, generator=gen), eps_cur=r(n, B, A), eps_nxt=r(n, B, A))
    mod.logged = {}
    mod.training_step(to_dev(batch, mod.device), 0, noise=to_dev(noise, mod.device))
    torch.cuda.synchronize()
    spec = R.Spec()
    P = O.require_grad_({k: v.clone() for k, v in params.items()}, frozen_prefixes=("target_q1.", "target_q2."))
    logs = {}
    ograds = R.ac_update(P, O.make_opts(P, spec), spec, batch["observations"], batch["next_observations"], batch["actions"],
                         reward.unsqueeze(-1), reward.unsqueeze(-1).clone(), noise, 0, logs)
    got = _logged(mod)
    assert set(logs) <= set(got), sorted(set(logs) - set(got))
    bad = check_logs(got, logs)
    bad += compare_with_oracle_grads(mod, ograds, GRAD_RTOL)
    sd = mod.state_dict()
    for k, v in P.items():
        if (sd[k].cpu() - v.detach()).abs().max().item() > RTOL * v.detach().abs().max().item() + PARAM_ATOL:
            bad.append(f"param {k}: max|d| {(sd[k].cpu() - v.detach()).abs().max().item():.3g}")
    assert not bad, "\n".join(bad[:25])


def test_action_decoder_act_without_gripper():
    """ActionDecoderLogistic.act with discrete_gripper False (reference :90-100,265-266): (B, 1, Da) actions - no gripper
    column - over three calls with the carried hidden state, against the restatement's forward + _sample on the same
    injected uniforms (f32: heads 1e-4, the sampled action where the Gumbel choice is clear)."""
    from tacorl_amd import synth
    from tacorl_amd.networks.action_decoder import ActionDecoderLogistic

    B, P_, E, H, Da, Kmix = 3, 16, K.STATE_DIM, 64, K.ACTION_DIM, 10
    ad = ActionDecoderLogistic(torch.device(DEV), state_dim=E, latent_plan_dim=P_, hidden_size=H, out_features=Da,
                               act_max_bound=[1.0] * Da, act_min_bound=[-1.0] * Da, discrete_gripper=False)
    W = {"action_decoder." + k: synth.param_values(k, v.shape, 81) * 3.0 for k, v in ad.blk.views.items()}
    with torch.no_grad():
        for k, v in ad.blk.views.items():
            v.copy_(W["action_decoder." + k])
    gen = torch.Generator().manual_seed(82)
    plan, emb = torch.tanh(torch.randn(B, P_, generator=gen)), torch.randn(B, 3, E, generator=gen)
    ra, rb = torch.rand(3, B, 1, Da, Kmix, generator=gen), torch.rand(3, B, 1, Da, generator=gen) * 0.8 + 0.1
    lp, ls, mm = R.action_decoder_fwd(W, "action_decoder.", plan, emb)  # (the RNN is causal: step t of the full pass)
    ad.clear_hidden_state()
    for t in range(3):
        a = ad.act(plan.to(DEV), emb[:, t:t + 1].to(DEV), noise=(ra[t], rb[t]))
        assert a.shape == (B, 1, Da)
        want = R.logistic_sample(lp[:, t:t + 1], ls[:, t:t + 1], mm[:, t:t + 1], ra[t], rb[t])
        score = lp[:, t:t + 1] - torch.log(-torch.log((1e-5 - (1.0 - 1e-5)) * ra[t] + (1.0 - 1e-5)))
        top = score.topk(2, -1).values
        clear = (top[..., 0] - top[..., 1]) > 1e-3
        assert clear.float().mean() > 0.9
        assert torch.allclose(a.cpu()[clear], want[clear], rtol=1e-4, atol=1e-5), (t, (a.cpu() - want).abs().max())
    assert ad.hidden_state.shape == (2, B, H)


# ---------------------------------------------------------------------------------------------- bf16 mode
def test_tacorl_d4rl_step_bf16_vs_rounded_restatement():
    from oracle import tacorl_oracle as O

    g = K.D4rlGolden("tacorl_d4rl_ad")
    mod = build_tacorl(g, compute="bf16")
    mod.load_state_dict(g.params(), strict=False)
    spec = R.Spec(finetune_action_decoder=True)
    P = R.require_grad_(g.params())
    opts = O.make_opts(P, spec)
    bad = []
    for step in range(g.cfg["steps"]):
        batch, noise = g.batch(step), g.noise(step)
        if step:
            resync_oracle(mod, P, opts)
        before = _snap(P)
        mod.logged = {}
        mod.training_step(to_dev(batch, mod.device), noise=to_dev(noise, mod.device))
        torch.cuda.synchronize()
        opts0 = copy.deepcopy(opts)
        with O.operand_rounding(torch.bfloat16):
            ologs, oplan, ograds = R.tacorl_step(P, opts, spec, batch, noise, 0)
            floor = gradient_floor(lambda Pp: R.tacorl_step(Pp, copy.deepcopy(opts0), spec, batch, noise, 0)[2], before, ograds)
        floor = _with_bf16_sensitivity(floor, ograds, R.tacorl_step(_snap(before), copy.deepcopy(opts0), spec, batch, noise, 0)[2])
        bad += _bf16_compare(mod, _logged(mod), ologs, ograds, before, P, step, mod.engine.action, oplan, floor)
    assert not bad, "\n".join(bad[:30])


def test_playlmp_d4rl_step_bf16_vs_rounded_restatement():
    from oracle import tacorl_oracle as O

    g = K.D4rlGolden("playlmp_d4rl")
    mod = build_playlmp(g, compute="bf16")
    mod.load_state_dict(g.params(), strict=False)
    P = O.require_grad_(g.params())
    opt = O.Adam([n for n in P], 1e-4)
    dp, bad = g.cfg["dropout_p"], []
    for step in range(g.cfg["steps"]):
        batch, nz = g.batch(step), g.noise(step)
        if step:
            resync_oracle(mod, P, opt)
        before = _snap(P)
        mod.logged = {}
        mod.training_step(to_dev(batch, mod.device), 0, noise=nz)
        torch.cuda.synchronize()
        opt0 = copy.deepcopy(opt)
        with O.operand_rounding(torch.bfloat16):
            ologs, ograds, oplan = R.playlmp_step(P, opt, batch, nz, dropout_p=dp)
            floor = gradient_floor(lambda Pp: R.playlmp_step(Pp, copy.deepcopy(opt0), batch, nz, dropout_p=dp)[1], before, ograds)
        floor = _with_bf16_sensitivity(floor, ograds, R.playlmp_step(_snap(before), copy.deepcopy(opt0), batch, nz, dropout_p=dp)[1])
        bad += _bf16_compare(mod, _logged(mod), ologs, ograds, before, P, step, mod.plan, oplan, floor)
    assert not bad, "\n".join(bad[:30])


# ---------------------------------------------------------------------------------------------- two ranks
def test_two_rank_shards_equal_the_full_batch_step():
    """TACORL-D4RL (frozen / fine-tuned action decoder) and PlayLMP-D4RL: two ranks on shards of 2 + 2 samples with sharded
    noise, graph segments around the all-reduces, against the single-rank step on B = 4 (tests/d4rl_shard_script.py)."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "d4rl_shard_script.py")]
    out = run_group(cmd, env, ROOT, timeout=300)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
