"""The bidirectional-RNN plan recognition (`plan_recognition=tanh_net`: reference plan_encoders/plan_recognition_tanh_net.py)
on the host: configuration checks, the reference's state-dict layout, checkpoint interchange, and an fp32 restatement of
the posterior that - patched over the oracle's transformer posterior - reproduces the reference's goldens (tools/
gen_birnn_golden.py).  That patched oracle is the yardstick tests/test_birnn_gpu.py holds the HIP path to."""
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import tacorl_oracle as O
from tests import cfg_util as C
from tests.golden_util import Golden, check_stats, spec_for

RTOL, GRAD_RTOL, PARAM_ATOL, TEMPERATURE_GRAD_RTOL = 2e-5, 5e-5, 1e-5, 2e-4  # test_oracle_golden.py's tolerances

TANH_NET = {"_target_": "tacorl.networks.plan_encoders.plan_recognition_tanh_net.PlanRecognitionTanhNetwork",
            "state_dim": None, "latent_plan_dim": 16, "birnn_dropout_p": 0.0, "min_std": 0.0001}


def tanh_net(latent=16, **over):
    return dict(TANH_NET, latent_plan_dim=latent, **over)


def strip(c):
    return {k: v for k, v in c.items() if k not in ("_target_", "_recursive_")}


# ------------------------------------------------------------------------------------------- restatement
def _rnn_direction(P, p, x, steps):
    """One direction of one nn.RNN(relu) layer from the zero state over the given time order; returns {t: h_t}."""
    xi = O._linear(x, P[p.format("weight_ih")], P[p.format("bias_ih")])
    h = torch.zeros(x.shape[0], xi.shape[-1], dtype=x.dtype)
    out = {}
    for t in steps:
        h = F.relu(xi[:, t] + O._linear(h, P[p.format("weight_hh")], P[p.format("bias_hh")]))
        out[t] = h
    return out


def birnn_posterior(P, pre, emb, n_heads=8, n_layers=2, min_std=1e-4, dropout=None):
    """PlanRecognitionTanhNetwork.forward (fp32): torch nn.RNN(relu, num_layers=2, bidirectional=True, batch_first=True)
    -> x[:, -1] -> mean_fc / softplus(variance_fc) + min_std.  emb (B,T,D) -> mu, std (B,A).  Every contraction goes through
    the oracle's _linear (operand_rounding applies).  The signature is the oracle's plan_recognition's (patched over it)."""
    assert dropout is None
    B, T, _ = emb.shape
    m = pre + "birnn_model.{}"
    with O._region("rnn"):
        f1 = _rnn_direction(P, m + "_l0", emb, range(T))
        r1 = _rnn_direction(P, m + "_l0_reverse", emb, reversed(range(T)))
        y1 = torch.stack([torch.cat([f1[t], r1[t]], dim=-1) for t in range(T)], dim=1)  # (B, T, 2H)
        f2 = _rnn_direction(P, m + "_l1", y1, range(T))[T - 1]
        r2 = _rnn_direction(P, m + "_l1_reverse", y1[:, T - 1:], [0])[0]  # layer 2 reverse at T-1: its first step
        x = torch.cat([f2, r2], dim=-1)
        mean = O._linear(x, P[pre + "mean_fc.weight"], P[pre + "mean_fc.bias"])
        std = F.softplus(O._linear(x, P[pre + "variance_fc.weight"], P[pre + "variance_fc.bias"])) + min_std
    return mean, std


@pytest.fixture
def birnn_oracle(monkeypatch):
    """The oracle with the bi-RNN posterior (playlmp_step and pr_latent_plan look plan_recognition up at call time)."""
    monkeypatch.setattr(O, "plan_recognition", birnn_posterior)
    return O


# ------------------------------------------------------------------------------------------- construction
def test_playlmp_builds_with_tanh_net_and_reference_names():
    from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP
    from tacorl_amd.networks.plan_recognition_birnn import PlanRecognitionBiRNN

    H, A = 256, 16
    mod = PlayLMP(**strip(C.playlmp_cfg(device="cpu", plan_recognition=tanh_net(A, hidden_dim=H))))
    assert isinstance(mod.pr, PlanRecognitionBiRNN)
    assert mod.pr.A == A and mod.pr.D == mod.pr.D_in == 32 and mod.pr.dropout_p == 0 and mod.pr.min_std == 1e-4
    rnn = torch.nn.RNN(32, H, num_layers=2, nonlinearity="relu", bidirectional=True, batch_first=True)
    exp = {f"plan_recognition.birnn_model.{k}": tuple(v.shape) for k, v in rnn.state_dict().items()}
    for head in ("mean_fc", "variance_fc"):
        exp.update({f"plan_recognition.{head}.{k}": tuple(v.shape) for k, v in torch.nn.Linear(2 * H, A).state_dict().items()})
    got = {k: tuple(v.shape) for k, v in mod.state_dict().items() if k.startswith("plan_recognition.")}
    assert got == exp
    # reference init: nn.RNN U(+-1/sqrt(H)) on every tensor, nn.Linear's default on the heads (none left at zero)
    sd = mod.state_dict()
    for k, v in sd.items():
        if k.startswith("plan_recognition.birnn_model."):
            assert 0.5 / H ** 0.5 < float(v.abs().max()) <= 1.0 / H ** 0.5, k
    assert 0 < float(sd["plan_recognition.mean_fc.weight"].abs().max()) <= 1.0 / (2 * H) ** 0.5


def test_plan_recognition_config_rejections():
    from tacorl_amd.modules import cfgcheck

    assert cfgcheck.check_plan_recognition(tanh_net(), "pr")[0] == "birnn"
    assert cfgcheck.check_plan_recognition(C.plan_recognition(16, 16), "pr")[0] == "transformer"
    with pytest.raises(NotImplementedError):
        cfgcheck.check_plan_recognition(tanh_net(birnn_dropout_p=0.1), "pr")
    with pytest.raises(NotImplementedError):
        cfgcheck.check_plan_recognition(tanh_net(num_layers=3), "pr")
    broken = {"_target_": "tacorl.networks.plan_encoders.plan_recognition_net.PlanRecognitionNetwork", "in_features": 32}
    with pytest.raises(NotImplementedError):
        cfgcheck.check_plan_recognition(broken, "pr")
    from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP

    with pytest.raises(NotImplementedError):
        PlayLMP(**strip(C.playlmp_cfg(device="cpu", plan_recognition=tanh_net(birnn_dropout_p=0.1, hidden_dim=64))))


def _write_tanh_run_dir(root, sd, latent=16):
    import yaml

    C.write_reference_run_dir(root, sd, latent=latent)
    p = os.path.join(root, ".hydra", "config.yaml")
    cfg = yaml.safe_load(open(p))
    cfg["module"]["plan_recognition"] = dict(TANH_NET, latent_plan_dim="${latent_plan_dim}")
    with open(p, "w") as f:
        yaml.safe_dump(cfg, f)


def test_tacorl_builds_from_a_tanh_net_run_directory(tmp_path):
    """TACORL(play_lmp_dir=...) over a reference-layout PlayLMP run directory that selected tanh_net (`${latent_plan_dim}`
    unresolved in its .hydra/config.yaml)."""
    from tacorl_amd.modules.tacorl.tacorl import TACORL
    from tacorl_amd.networks.plan_recognition_birnn import PlanRecognitionBiRNN

    g = Golden("tacorl_birnn_q")
    sd = C.lmp_state_dict_from_tacorl(g.params())
    _write_tanh_run_dir(str(tmp_path), sd)
    mod = TACORL(play_lmp_dir=str(tmp_path), **strip(C.tacorl_cfg(device="cpu", finetune_action_decoder=False)))
    assert isinstance(mod.pr, PlanRecognitionBiRNN) and mod.pr.latent_plan_dim == 16
    assert sorted(n for n, _ in mod.named_parameters()) == sorted(g.names)
    got = mod.state_dict()
    for k in ("plan_recognition.birnn_model.weight_ih_l1_reverse", "plan_recognition.birnn_model.bias_hh_l0",
              "plan_recognition.variance_fc.weight", "action_decoder.rnn.weight_hh_l1"):
        assert torch.equal(got[k].cpu(), sd[k]), k


# ------------------------------------------------------------------------------------------- restatement pin
def _check_grads(got, exp):  # (a soft-argmax temperature's gradient: see test_oracle_golden.py)
    temp = {k: v for k, v in exp.items() if k.endswith(".temperature")}
    rest = {k: v for k, v in exp.items() if k not in temp}
    return (check_stats(got, rest, rtol=GRAD_RTOL, what="grad ")
            + check_stats(got, temp, rtol=TEMPERATURE_GRAD_RTOL, what="grad "))


def _check_logs(got, exp, rtol=RTOL):
    return [f"{k}: {got[k]:.8g} vs {v:.8g}" for k, v in exp.items() if k in got and abs(got[k] - v) > rtol * max(abs(v), 1e-3)]


def test_restatement_reproduces_playlmp_birnn(birnn_oracle):
    g = Golden("playlmp_birnn")
    assert g.cfg["plan_recognition"] == "tanh_net"
    P = O.require_grad_(g.params())
    opt = O.Adam([n for n in P], 1e-4)
    for step in range(g.cfg["steps"]):
        logs, grads = O.playlmp_step(P, opt, g.batch(step), g.noise(step), sorted(g.cams))
        bad = _check_logs(logs, g.logged(step))
        bad += _check_grads(grads, g.stats(step, "grad"))
        bad += check_stats(P, g.stats(step, "param"), rtol=RTOL, atol=PARAM_ATOL, what="param ")
        assert not bad, "\n".join(bad[:20])
    assert any(k.startswith("plan_recognition.birnn_model.") for k in g.stats(0, "grad"))


@pytest.mark.parametrize("name", ["tacorl_birnn_q", "val_tacorl_birnn"])
def test_restatement_reproduces_tacorl_birnn(birnn_oracle, name):
    g = Golden(name)
    spec = spec_for(g)
    P = O.require_grad_(g.params(), frozen_prefixes=("perceptual_encoder.", "plan_recognition."))
    opts = O.make_opts(P, spec)
    if g.cfg.get("validate"):
        with torch.no_grad():
            plan, _ = O.pr_latent_plan(P, g.batch(0)["states"], spec, g.noise(0)["eps_pr"])
        assert torch.allclose(plan, g.latent_plan(0), rtol=1e-5, atol=1e-6)
        return
    for step in range(g.cfg["steps"]):
        logs, plan, grads = O.tacorl_step(P, opts, spec, g.batch(step), g.noise(step), g.cfg["epoch"])
        assert torch.allclose(plan, g.latent_plan(step), rtol=1e-5, atol=1e-6)
        bad = _check_logs(logs, g.logged(step))
        bad += _check_grads(grads, g.stats(step, "grad"))
        bad += check_stats(P, g.stats(step, "param"), rtol=RTOL, atol=PARAM_ATOL, what="param ")
        assert not bad, "\n".join(bad[:20])
