"""Pin the CPU oracle (oracle/tacorl_oracle.py) against goldens produced by the
unmodified reference (oracle/gen_golden.py).  CPU-only; no reference access needed."""
import numpy as np
import pytest
import torch

from oracle import tacorl_oracle as O
from tests.golden_util import Golden, check_stats, spec_for

PARAM_ATOL = 1e-5  # ~3% of one Adam update (lr 3e-4): near-zero grads flip under g/(|g|+eps)
RTOL = 2e-5  # fp32 re-association (de-duplicated encoders, fused grads) stays below this
GRAD_RTOL = 5e-5
# A spatial soft-argmax temperature's gradient is one fp32 sum over every activation of its encoder, most of which cancels,
# so its last digits follow the CPU's vector kernels: on cql_n32 step 1 the reference's own fp32 value lies 7.7e-5 (relative)
# from the fp64 evaluation, and the oracle's AVX2 / AVX-512 kernels land 7.0e-5 / 1.6e-5 from the reference's.
TEMPERATURE_GRAD_RTOL = 2e-4


def _check_grads(got, exp):
    temp = {k: v for k, v in exp.items() if k.endswith(".temperature")}
    rest = {k: v for k, v in exp.items() if k not in temp}
    return (check_stats(got, rest, rtol=GRAD_RTOL, what="grad ")
            + check_stats(got, temp, rtol=TEMPERATURE_GRAD_RTOL, what="grad "))


def _check_logs(got, exp, rtol=RTOL):
    bad = []
    for k, v in exp.items():
        if k not in got:
            continue
        if abs(got[k] - v) > rtol * max(abs(v), 1e-3):
            bad.append(f"{k}: {got[k]:.8g} vs {v:.8g}")
    return bad


@pytest.mark.parametrize("name", ["tacorl_q", "tacorl_bc_ad", "tacorl_dualcam", "tacorl_c4", "tacorl_q_ad"])
@pytest.mark.parametrize("faithful", [False, True])
def test_tacorl_step_matches_reference(name, faithful):
    if faithful and name != "tacorl_q":
        pytest.skip("faithful schedule checked once")
    g = Golden(name)
    spec = spec_for(g)
    P = O.require_grad_(g.params(), frozen_prefixes=("perceptual_encoder.", "plan_recognition."))
    opts = O.make_opts(P, spec)
    for step in range(g.cfg["steps"]):
        logs, plan, grads = O.tacorl_step(P, opts, spec, g.batch(step), g.noise(step), g.cfg["epoch"],
                                          faithful=faithful)
        exp = g.logged(step)
        assert set(exp) - set(logs) == set(), set(exp) - set(logs)
        bad = _check_logs(logs, exp)
        assert torch.allclose(plan, g.latent_plan(step), rtol=1e-5, atol=1e-6)
        bad += _check_grads(grads, g.stats(step, "grad"))
        bad += check_stats(P, g.stats(step, "param"), rtol=RTOL, atol=PARAM_ATOL, what="param ")
        assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("name", ["cql_q", "cql_bc", "cql_n32"])
def test_cql_step_matches_reference(name):
    g = Golden(name)
    spec = spec_for(g)
    P = O.require_grad_(g.params())
    opts = O.make_opts(P, spec)
    for step in range(g.cfg["steps"]):
        logs, grads = O.cql_step(P, opts, spec, g.batch(step), g.noise(step), g.cfg["epoch"])
        bad = _check_logs(logs, g.logged(step))
        bad += _check_grads(grads, g.stats(step, "grad"))
        bad += check_stats(P, g.stats(step, "param"), rtol=RTOL, atol=PARAM_ATOL, what="param ")
        assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("name", ["playlmp", "playlmp_dropout"])
def test_playlmp_step_matches_reference(name):
    g = Golden(name)
    P = O.require_grad_(g.params())
    opt = O.Adam([n for n in P], 1e-4)
    for step in range(g.cfg["steps"]):
        logs, grads = O.playlmp_step(P, opt, g.batch(step), g.noise(step), sorted(g.cams),
                                     dropout_p=g.cfg.get("dropout_p", 0.0))
        bad = _check_logs(logs, g.logged(step))
        bad += _check_grads(grads, g.stats(step, "grad"))
        bad += check_stats(P, g.stats(step, "param"), rtol=RTOL, atol=PARAM_ATOL, what="param ")
        assert not bad, "\n".join(bad[:20])


def test_golden_param_layout_is_reference_layout():
    """State-dict key layout the boundary must keep (SURVEY 8a note 9)."""
    g = Golden("tacorl_q")
    names = set(g.names)
    for k in ("actor.actor.policy.fc_layers.0.weight", "actor.encoder.networks.rgb_static.model.0.weight",
              "actor.encoder.networks.rgb_static.model.6.temperature", "q1.critic.Q.out.weight",
              "target_q2.goal_encoder.mlp.4.bias", "perceptual_encoder.networks.rgb_static.fc_layers.3.weight",
              "plan_recognition.transformer_encoder.layers.1.linear2.weight", "action_decoder.rnn.weight_hh_l1",
              "log_alpha", "log_alpha_prime"):
        assert k in names, k
    assert sum(int(np.prod(s)) for n, s in zip(g.names, g.shapes) if n.startswith("q1.")) == 352226


def test_rollout_surface_matches_reference():
    """actor.get_actions (deterministic / sampled), the frozen LMP encoder's state and three
    action_decoder.act steps with the carried hidden state, as the reference's rollout manager calls them."""
    g = Golden("rollout_tacorl")
    z, P, cams = g.z, g.params(), sorted(g.cams)
    spec = O.ACSpec(cams=cams, goal_cams=cams, action_dim=g.cfg["latent"], discrete_gripper=False, target_entropy=-7.0,
                    ac_cams=cams, pr_cams=cams)
    batch, tape = g.batch(0), g.tape(0)
    assert [k for k, _ in tape] == ["normal"] + ["rand"] * 6
    obs0 = {c: v[:, 0] for c, v in batch["states"].items()}
    with torch.no_grad():
        plan, lp = O.actor_get_actions(P, "actor.", obs0, batch["goal"], spec, deterministic=True)
        assert torch.allclose(plan, torch.from_numpy(z["plan"]), rtol=1e-5, atol=1e-6) and float(lp.abs().max()) == 0.0
        ps, lps = O.actor_get_actions(P, "actor.", obs0, batch["goal"], spec, noise={"eps": tape[0][1]})
        assert torch.allclose(ps, torch.from_numpy(z["plan_sampled"]), rtol=1e-5, atol=1e-6)
        assert torch.allclose(lps, torch.from_numpy(z["logpi_sampled"]), rtol=1e-5, atol=1e-5)
        h = None
        for t in range(3):
            emb = O.late_fusion(P, "perceptual_encoder.", {c: v[:, t] for c, v in batch["states"].items()}, cams)
            assert torch.allclose(emb, torch.from_numpy(z["ad_state"][t]), rtol=1e-5, atol=1e-6)
            a, h = O.action_decoder_act(P, "action_decoder.", plan, emb.unsqueeze(1), h, tape[1 + 2 * t][1], tape[2 + 2 * t][1])
            assert torch.allclose(a, torch.from_numpy(z["actions"][t]), rtol=1e-4, atol=1e-5), t
        assert torch.allclose(h, torch.from_numpy(z["hidden"]), rtol=1e-5, atol=1e-6)


def test_rollout_discrete_gripper_actions_match_reference():
    g = Golden("rollout_cql")
    z, P, cams = g.z, g.params(), sorted(g.cams)
    spec = O.ACSpec(cams=cams, goal_cams=cams, action_dim=7, discrete_gripper=True, target_entropy=-7.0)
    o, tape = g.batch(0)["observations"], g.tape(0)
    assert [k for k, _ in tape] == ["normal", "uniform01", "normal", "rand"]
    with torch.no_grad():
        a, _ = O.actor_get_actions(P, "actor.", o["observation"], o["goal"], spec, deterministic=True)
        assert torch.allclose(a, torch.from_numpy(z["act_det"]), rtol=1e-5, atol=1e-6)
        a, lp = O.actor_get_actions(P, "actor.", o["observation"], o["goal"], spec, noise={"eps": tape[0][1], "gumbel_u": tape[1][1]})
        assert torch.allclose(a, torch.from_numpy(z["act_sample"]), rtol=1e-5, atol=1e-6)
        assert torch.allclose(lp, torch.from_numpy(z["logpi_sample"]), rtol=1e-5, atol=1e-5)
        a, lp = O.actor_get_actions(P, "actor.", o["observation"], o["goal"], spec, reparameterize=True,
                                    noise={"eps": tape[2][1], "gumbel_u": tape[3][1]})
        assert torch.allclose(a, torch.from_numpy(z["act_rsample"]), rtol=1e-5, atol=1e-6)
        assert torch.allclose(lp, torch.from_numpy(z["logpi_rsample"]), rtol=1e-5, atol=1e-5)


# ---- free-running trajectories (round 5): no re-synchronisation between steps ---------------------------
# The reference ran 12 (TACORL, action-decoder fine-tuning on, current_epoch 4 -> 5 after step 6: the BC -> Q switch of the
# actor loss, cql_offline_lightning.py:459-466) / 8 (PlayLMP) optimiser steps from one initial state; the oracle does the
# same from the same state with the same noise tape, on its OWN trajectory.  What this pins beyond the 1-2 step fixtures:
# Adam's bias-correction counters and moments, the Polyak drift of the target critics, the phase switch.  Two fp32
# implementations do not stay bit-close over many Adam steps (the first update is lr * sign(g): elements whose gradient
# is ~0 move by +-lr on summation order alone) - the tolerances below are the measured divergence of this oracle from
# the reference with a margin (measured, printed by the test: TACORL <= 6.5e-7 over all 12 steps; PlayLMP 0 at step 1
# growing to 4.4e-5 at step 8 - its RNN weights take the lr * sign(g) updates).
TRAJ_LOG_RTOL = {"tacorl": 1e-5, "playlmp": 3e-4}


def _traj_divergence(got, exp):
    return max(abs(got[k] - v) / max(abs(v), 1e-2) for k, v in exp.items() if k in got)


def test_tacorl_trajectory_matches_reference():
    g = Golden("tacorl_traj")
    spec = spec_for(g)
    P = O.require_grad_(g.params(), frozen_prefixes=("perceptual_encoder.", "plan_recognition."))
    opts = O.make_opts(P, spec)
    worst = []
    for step in range(g.cfg["steps"]):
        epoch = g.cfg["epochs"][step]
        logs, plan, _ = O.tacorl_step(P, opts, spec, g.batch(step), g.noise(step), epoch)
        exp = g.logged(step)
        assert set(exp) - set(logs) == set(), set(exp) - set(logs)
        worst.append(_traj_divergence(logs, exp))
        assert torch.allclose(plan, g.latent_plan(step), rtol=1e-5, atol=1e-6)  # (frozen LMP: no drift at all)
        assert worst[-1] < TRAJ_LOG_RTOL["tacorl"], (step, worst, _check_logs(logs, exp, TRAJ_LOG_RTOL["tacorl"]))
        if step in g.cfg["param_steps"]:
            bad = check_stats(P, g.stats(step, "param"), rtol=1e-4, atol=3e-5 * (1 + step), what=f"step {step} param ")
            assert not bad, "\n".join(bad[:20])
    print("tacorl_traj: worst relative log divergence per step", [f"{w:.1e}" for w in worst])
    # the actor loss changed form at the switch (BC: alpha*logp - logp(a_data); Q: alpha*logp - min Q)
    assert g.logged(5)["actor_loss"] > 0 > g.logged(6)["actor_loss"]
    # Adam counters: every optimiser of the reference stepped 12 times; the oracle's too
    import json
    assert json.loads(str(g.z["adam_steps"])) == [[12]] * 6
    assert {o.t for o in opts.values()} == {12}


def test_playlmp_trajectory_matches_reference():
    g = Golden("playlmp_traj")
    P = O.require_grad_(g.params())
    opt = O.Adam([n for n in P], 1e-4)
    worst = []
    for step in range(g.cfg["steps"]):
        logs, _ = O.playlmp_step(P, opt, g.batch(step), g.noise(step), sorted(g.cams))
        exp = g.logged(step)
        exp = {k: v for k, v in exp.items() if "gripper_accuracy" not in k}  # (a count over 60 samples: one flip = 1.7 %)
        worst.append(_traj_divergence(logs, exp))
        assert worst[-1] < TRAJ_LOG_RTOL["playlmp"], (step, worst, _check_logs(logs, exp, TRAJ_LOG_RTOL["playlmp"]))
        if step in g.cfg["param_steps"]:
            bad = check_stats(P, g.stats(step, "param"), rtol=1e-4, atol=3e-5 * (1 + step), what=f"step {step} param ")
            assert not bad, "\n".join(bad[:20])
    print("playlmp_traj: worst relative log divergence per step", [f"{w:.1e}" for w in worst])
    assert opt.t == 8
