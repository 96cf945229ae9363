"""The D4RL module configs as Hydra would hand them to `instantiate` after composing the reference's YAMLs
(config/module/{play_lmp_d4rl,tacorl_d4rl}.yaml with their defaults lists resolved; `_recursive_: False`, so sub-configs stay
dicts), and the loader of the goldens tools/gen_d4rl_golden.py writes."""
from tacorl_amd import synth
from tests import cfg_util as C
from tests.golden_util import Golden

ENV = "antmaze-large-diverse-v0"
STATE_DIM, ACTION_DIM, GOAL_DIM = 29, 8, 2


def playlmp_d4rl_cfg(latent=16, T=8, device="cpu", dropout_p=0.1, **over):
    cfg = {"_target_": "tacorl_amd.modules.play_lmp.play_lmp_d4rl.PlayLMP", "_recursive_": False, "plan_proposal": C.ACTOR,
           "plan_recognition": C.plan_recognition(latent, T, dropout_p),
           # config/module/play_lmp_d4rl.yaml:11-12 on top of networks/action_decoder/logistic.yaml
           "action_decoder": dict(C.action_decoder(latent), discrete_gripper=False),
           "lr": 1e-4, "kl_beta": 1e-3, "d4rl_env": ENV, "device": device}
    cfg.update(over)
    return cfg


# config/module/tacorl_d4rl.yaml:8-26
TACORL_D4RL = {"finetune_action_decoder": True, "action_decoder_lr": 3e-4, "actor_lr": 1e-4, "critic_lr": 3e-4, "discount": 0.95,
               "conservative_weight": 1.0, "reward_scale": 10.0, "n_action_samples": 4, "with_lagrange": True,
               "deterministic_backup": True, "bc_epochs": 0, "with_vib": False, "vib_coefficient": 0.03}


def tacorl_d4rl_cfg(device="cpu", **over):
    cfg = {"_target_": "tacorl_amd.modules.tacorl.tacorl_d4rl.TACORL", "_recursive_": False, "critic": C.CRITIC,
           "d4rl_env": ENV, "device": device, **TACORL_D4RL}
    cfg.update(over)
    return cfg


def cql_d4rl_cfg(device="cpu", **over):
    cfg = {"_target_": "tacorl_amd.modules.cql.cql_offline_lightning_d4rl.CQL_Offline", "_recursive_": False,
           "actor": C.ACTOR, "critic": C.CRITIC, "d4rl_env": ENV, "device": device,
           **{k: v for k, v in TACORL_D4RL.items() if k not in ("finetune_action_decoder", "action_decoder_lr")}}
    cfg.update(over)
    return cfg


def build(cfg):
    """hydra.utils.instantiate(cfg) for a `_recursive_: False` module config."""
    import importlib

    cfg = dict(cfg)
    mod, cls = cfg.pop("_target_").rsplit(".", 1)
    cfg.pop("_recursive_", None)
    return getattr(importlib.import_module(mod), cls)(**cfg)


def write_reference_run_dir(root, lmp_state_dict, latent=16, T=8):
    """A PlayLMP-D4RL run directory as the reference's training leaves it: Hydra's `.hydra/config.yaml` with its interpolations
    unresolved (`${latent_plan_dim}`, `${datamodule.dataset.max_window_size}`, `${d4rl_env}` - config/experiment/
    play_lmp_d4rl.yaml) and a PL checkpoint under model_ckpts/: what `load_pl_module_from_checkpoint` consumes."""
    import os

    import torch
    import yaml

    pr = dict(C.plan_recognition(latent, T, 0.1), latent_plan_dim="${latent_plan_dim}",
              max_position_embeddings="${datamodule.dataset.max_window_size}")
    ad = dict(C.action_decoder(latent), latent_plan_dim="${latent_plan_dim}", discrete_gripper=False)
    cfg = {"latent_plan_dim": latent, "d4rl_env": ENV, "seed": 42,
           "datamodule": {"dataset": {"max_window_size": T, "min_window_size": T, "d4rl_env": "${d4rl_env}"}},
           "module": {"_target_": "tacorl.modules.play_lmp.play_lmp_d4rl.PlayLMP", "_recursive_": False, "plan_proposal": C.ACTOR,
                      "plan_recognition": pr, "action_decoder": ad, "lr": 1e-4, "kl_beta": 1e-3, "d4rl_env": "${d4rl_env}"}}
    os.makedirs(os.path.join(root, ".hydra"), exist_ok=True)
    os.makedirs(os.path.join(root, "model_ckpts"), exist_ok=True)
    with open(os.path.join(root, ".hydra", "config.yaml"), "w") as f:
        yaml.safe_dump(cfg, f)
    torch.save({"epoch": 3, "global_step": 30, "pytorch-lightning_version": "1.6.5", "state_dict": dict(lmp_state_dict),
                "hyper_parameters": {"lr": 1e-4}}, os.path.join(root, "model_ckpts", "last.ckpt"))
    return root


class D4rlGolden(Golden):
    def batch(self, step, B=None):
        return synth.make_d4rl_window_batch(self.cfg["seed"] * 100 + step, B or self.cfg["B"], self.cfg["T"], STATE_DIM, ACTION_DIM)

    def noise(self, step):
        """The recorded draws by name.  PlayLMP: the plan recognition's keep masks, the rsample, the uniform random plan;
        TACORL: SURVEY 8a note 1 without images."""
        t = self.tape(step)
        if self.cfg["kind"] == "playlmp_d4rl":
            nd = sum(1 for k, _ in t if k == "dropout")
            assert [k for k, _ in t] == ["dropout"] * nd + ["normal", "uniform01"]
            nz = dict(eps_plan=t[nd][1], u_plan=t[nd + 1][1])
            if nd:
                nz["dropout"] = [m for _, m in t[:nd]]
            return nz
        assert [k for k, _ in t] == ["normal", "normal", "normal", "uniform01", "normal", "normal"]
        return dict(zip(["eps_pr", "eps_pi", "eps_next", "u_rand", "eps_cur", "eps_nxt"], [v for _, v in t]))
