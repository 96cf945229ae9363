"""CPU side of the vector-observation (D4RL) family.

1. tests/d4rl_ref.py - the plain-torch restatement the GPU tests compare against - reproduces every golden that
   tools/gen_d4rl_golden.py recorded from the unmodified reference: logged scalars, sampled plans, gradient and parameter
   fingerprints, at the tolerances tests/test_oracle_golden.py applies to the image restatements.
2. The three module classes build on device="cpu" from configs as Hydra hands them over, with the reference's optimiser lists
   and state-dict keys; what is out of scope raises."""
import pytest
import torch

from oracle import tacorl_oracle as O
from tests import d4rl_cfg as K
from tests import d4rl_ref as R
from tests.golden_util import check_stats
from tests.test_oracle_golden import GRAD_RTOL, PARAM_ATOL, RTOL, _check_logs


def _spec(g):
    return R.Spec(finetune_action_decoder=g.cfg["finetune_ad"])


@pytest.mark.parametrize("name", ["tacorl_d4rl_q", "tacorl_d4rl_ad"])
def test_tacorl_d4rl_step_matches_reference(name):
    g = K.D4rlGolden(name)
    spec = _spec(g)
    P = R.require_grad_(g.params())
    opts = O.make_opts(P, spec)
    for step in range(g.cfg["steps"]):
        batch = g.batch(step)
        assert batch["goal_reached"].any() and not batch["goal_reached"].all()
        logs, plan, grads = R.tacorl_step(P, opts, spec, batch, g.noise(step), 0)
        exp = g.logged(step)
        assert set(exp) - set(logs) == set(), set(exp) - set(logs)
        bad = _check_logs(logs, exp)
        assert torch.allclose(plan, g.latent_plan(step), rtol=1e-5, atol=1e-6)
        exp_g = g.stats(step, "grad")
        assert exp_g and (name != "tacorl_d4rl_ad" or any(k.startswith("action_decoder.") for k in exp_g))
        bad += check_stats(grads, exp_g, rtol=GRAD_RTOL, what="grad ")
        bad += check_stats(P, g.stats(step, "param"), rtol=RTOL, atol=PARAM_ATOL, what="param ")
        assert not bad, "\n".join(bad[:20])


def test_tacorl_d4rl_validation_matches_reference():
    g = K.D4rlGolden("val_tacorl_d4rl")
    spec = _spec(g)
    P = R.require_grad_(g.params())
    logs, plan, grads = R.tacorl_step(P, O.make_opts(P, spec), spec, g.batch(0), g.noise(0), 0, optimize=False)
    exp = g.logged(0)
    assert set(exp) - set(logs) == set() and not grads
    assert torch.allclose(plan, g.latent_plan(0), rtol=1e-5, atol=1e-6)
    bad = _check_logs(logs, exp)
    assert not bad, "\n".join(bad)
    assert all(torch.equal(v, g.params()[k]) for k, v in P.items())  # nothing moved


def test_playlmp_d4rl_step_matches_reference():
    g = K.D4rlGolden("playlmp_d4rl")
    P = O.require_grad_(g.params())
    opt = O.Adam([n for n in P], 1e-4)
    for step in range(g.cfg["steps"]):
        logs, grads, _ = R.playlmp_step(P, opt, g.batch(step), g.noise(step), dropout_p=g.cfg["dropout_p"])
        exp = g.logged(step)
        assert set(exp) - set(logs) == set(), set(exp) - set(logs)
        bad = _check_logs(logs, exp)
        bad += check_stats(grads, g.stats(step, "grad"), rtol=GRAD_RTOL, what="grad ")
        bad += check_stats(P, g.stats(step, "param"), rtol=RTOL, atol=PARAM_ATOL, what="param ")
        assert not bad, "\n".join(bad[:20])


def test_golden_batches_reach_the_decoder_edge_branches():
    """Every golden batch holds actions on and just inside both bounds (the x < -0.999 and x > 0.999 branches of the decoder's
    likelihood) and inside them, and both values of goal_reached."""
    for name in ("playlmp_d4rl", "tacorl_d4rl_q", "tacorl_d4rl_ad", "val_tacorl_d4rl"):
        g = K.D4rlGolden(name)
        for step in range(g.cfg["steps"]):
            b = g.batch(step)
            a = b["actions"][:, :-1]
            assert (a < -0.999).any() and (a > 0.999).any() and ((a > -0.999) & (a < 0.999)).any()
            inside = torch.tensor(0.9995)  # (fp32)
            assert (a == -inside).any() and (a == inside).any() and (a == 1.0).any() and (a == -1.0).any()
            assert b["goal_reached"].any() and not b["goal_reached"].all()


# --------------------------------------------------------------------------------------------- construction
def _keys_and_shapes(mod):
    return {k: list(v.shape) for k, v in mod.named_parameters()}


def test_playlmp_d4rl_builds_on_cpu():
    g = K.D4rlGolden("playlmp_d4rl")
    lmp = K.build(K.playlmp_d4rl_cfg())
    assert _keys_and_shapes(lmp) == dict(zip(g.names, g.shapes))
    assert list(_keys_and_shapes(lmp)) == g.names  # (the reference's registration order too)
    from tacorl_amd.lightning import BlockAdam

    opt = lmp.configure_optimizers()
    assert isinstance(opt, BlockAdam) and opt.lr == 1e-4
    assert not any("gripper" in k for k in lmp.state_dict())
    assert lmp.state_dict()["action_decoder.action_max_bound"].shape == (1, 1, 8, 10)


@pytest.mark.parametrize("finetune,golden,n_opt", [(True, "tacorl_d4rl_ad", 6), (False, "tacorl_d4rl_q", 5)])
def test_tacorl_d4rl_builds_on_cpu(finetune, golden, n_opt):
    g = K.D4rlGolden(golden)
    t = K.build(K.tacorl_d4rl_cfg(play_lmp=K.build(K.playlmp_d4rl_cfg()), finetune_action_decoder=finetune))
    got = _keys_and_shapes(t)
    assert got == dict(zip(g.names, g.shapes))
    assert {k for k, p in t.named_parameters() if not p.requires_grad} == {n for n, r in zip(g.names, g.requires_grad) if not r}
    for k in ("actor.policy.fc_layers.0.weight", "q1.Q.out.weight", "target_q2.Q.fc_layers.2.bias", "log_alpha",
              "log_alpha_prime", "plan_recognition.transformer_encoder.layers.1.linear2.weight", "action_decoder.rnn.weight_hh_l1"):
        assert k in got, k
    assert not any(k.startswith(("actor.actor.", "actor.encoder", "perceptual_encoder")) or "gripper" in k for k in got)
    assert got["actor.policy.fc_layers.0.weight"] == [256, 31] and got["q1.Q.fc_layers.0.weight"] == [256, 31 + 16]
    opts = t.configure_optimizers()
    assert [o.name for o in opts] == ["alpha", "actor", "q1", "q2", "alpha_prime"] + (["action_decoder"] if finetune else [])
    assert len(opts) == n_opt
    assert [o.lr for o in opts] == [1e-4, 1e-4, 3e-4, 3e-4, 3e-4] + ([3e-4] if finetune else [])
    # the entropy target is the ENVIRONMENT's action dimension although the RL action is the 16-d plan (tacorl_d4rl.py, :76-78)
    assert t.target_entropy == -8.0 and t.engine.hp["target_entropy"] == -8.0 and t.engine.A == 16
    e = t.engine
    e.ensure_batch(2, 8)
    assert e.S["a"] is e.S["q1"] is e.S["q2"] and e.S["a_nx"] is e.S["tq1"] is e.S["tq2"] and e.S["a"] is not e.S["a_nx"]
    assert not hasattr(e, "enc_out") and not hasattr(e, "X3") and e.enc_cams == []


def test_tacorl_d4rl_loads_its_lmp_from_a_run_directory(tmp_path):
    """TACORL(play_lmp_dir=...): the resolved Hydra config + last.ckpt of a PlayLMP-D4RL run, as the image module loads its LMP;
    the actor is the checkpoint's plan proposal, the plan recognition and the decoder are the checkpoint's."""
    from tacorl_amd import synth

    src = K.build(K.playlmp_d4rl_cfg())
    synth.fill_params_(src, 5)
    sd = {k: v.detach().clone() for k, v in src.state_dict().items()}
    assert "action_decoder.ones" in sd and "action_decoder.gripper_bounds" not in sd
    run = K.write_reference_run_dir(str(tmp_path / "lmp_d4rl"), sd)
    t = K.build(K.tacorl_d4rl_cfg(play_lmp_dir=run))
    got = t.state_dict()
    for k, v in sd.items():
        name = "actor." + k[len("plan_proposal."):] if k.startswith("plan_proposal.") else k
        assert torch.equal(got[name], v), name
    assert t.pr.dropout_p == 0.1 and t.pr.T_max == 8 and t.ad.Da == 8 and not t.ad.discrete_gripper
    assert torch.equal(got["target_q1.Q.out.weight"], got["q1.Q.out.weight"])
    with pytest.raises(ValueError):
        K.build(K.tacorl_d4rl_cfg(play_lmp_dir=str(tmp_path / "nowhere")))


def test_cql_d4rl_builds_on_cpu():
    c = K.build(K.cql_d4rl_cfg())
    keys = _keys_and_shapes(c)
    assert keys["actor.policy.fc_layers.0.weight"] == [256, 31] and keys["q1.Q.fc_layers.0.weight"] == [256, 39]
    assert keys["actor.policy.fc_mean.weight"] == [8, 256] and "target_q1.Q.out.bias" in keys
    assert [o.name for o in c.configure_optimizers()] == ["alpha", "actor", "q1", "q2", "alpha_prime"]
    assert len(K.build(K.cql_d4rl_cfg(with_lagrange=False)).configure_optimizers()) == 4
    assert c.target_entropy == -8.0


def test_env_table_and_overrides():
    from tacorl_amd.modules.d4rl_env import env_dims

    assert env_dims("antmaze-umaze-v2") == (29, 8, 1.0) and env_dims("antmaze-medium-play-v0") == (29, 8, 1.0)
    assert env_dims("antmaze-large-diverse-v0", state_dim=11, action_dim=3) == (11, 3, 1.0)
    assert env_dims("my-env-v0", state_dim=11, action_dim=3) == (11, 3, 1.0)
    for cfg in (K.cql_d4rl_cfg(d4rl_env="hopper-medium-v2"), K.playlmp_d4rl_cfg(d4rl_env="hopper-medium-v2")):
        with pytest.raises(ValueError):
            K.build(cfg)
    with pytest.raises(ValueError):
        K.build(K.cql_d4rl_cfg(d4rl_env="hopper-medium-v2", state_dim=11))  # (both are needed)
    small = K.build(K.cql_d4rl_cfg(d4rl_env="my-env-v0", state_dim=11, action_dim=3))
    assert _keys_and_shapes(small)["actor.policy.fc_layers.0.weight"] == [256, 13] and small.target_entropy == -3.0


def test_out_of_scope_options_raise():
    lmp = K.build(K.playlmp_d4rl_cfg())
    for over in (dict(with_dr3=True), dict(with_vib=True)):
        with pytest.raises(NotImplementedError):
            K.build(K.cql_d4rl_cfg(**over))
        with pytest.raises(NotImplementedError):
            K.build(K.tacorl_d4rl_cfg(play_lmp=lmp, **over))
    with pytest.raises(NotImplementedError):  # an unknown sub-config option
        K.build(K.cql_d4rl_cfg(critic=dict(K.C.CRITIC, q_network=dict(K.C.CRITIC["q_network"], with_dropout=True))))
    with pytest.raises(NotImplementedError):
        K.build(K.playlmp_d4rl_cfg(plan_recognition=dict(K.C.plan_recognition(16, 8), encoder_normalize=True)))
    with pytest.raises(NotImplementedError):
        K.build(K.playlmp_d4rl_cfg(action_decoder=dict(K.C.action_decoder(16), discrete_gripper=False, policy_rnn_dropout_p=0.1)))


def test_nogo_imports():
    """Nothing of the D4RL family imports gym or d4rl."""
    import sys

    K.build(K.tacorl_d4rl_cfg(play_lmp=K.build(K.playlmp_d4rl_cfg())))
    assert "gym" not in sys.modules and "d4rl" not in sys.modules


def test_action_decoder_without_gripper_head():
    from tacorl_amd.networks.action_decoder import ActionDecoderLogistic

    kw = dict(state_dim=29, latent_plan_dim=16, hidden_size=64, out_features=8, act_max_bound=[1.0] * 8, act_min_bound=[-1.0] * 8)
    ad = ActionDecoderLogistic("cpu", discrete_gripper=False, **kw)
    assert (ad.Da, ad.AW, ad.NH) == (8, 8, 240)
    assert not any("gripper" in k for k in list(ad.blk.views) + list(ad.buffers))
    assert ad.blk.views["rnn.weight_ih_l0"].shape == (64, 45) and ad.blk.views["mean_fc.weight"].shape == (80, 64)
    assert ad.buffers["action_max_bound"].shape == (1, 1, 8, 10)
    # the three heads' weights and biases are back to back (one GEMM, one bias vector)
    o = ad.blk.off
    assert o["log_scale_fc.weight"][0] == o["mean_fc.weight"][0] + 80 * 64 and o["prob_fc.bias"][0] == o["mean_fc.bias"][0] + 160
    grip = ActionDecoderLogistic("cpu", discrete_gripper=True, **dict(kw, out_features=7, act_max_bound=[1.0] * 7, act_min_bound=[-1.0] * 7))
    assert (grip.Da, grip.AW, grip.NH) == (6, 7, 182) and "gripper_fc.weight" in grip.blk.views and "gripper_bounds" in grip.buffers
    with pytest.raises(ValueError):
        ActionDecoderLogistic("cpu", discrete_gripper=False, **dict(kw, act_max_bound=[1.0] * 7))
