"""Shared by the relay-imitation-learning tests and tools/gen_ril_golden.py: the synthetic batch (rebuilt from a seed, as
tacorl_amd.synth's batches are), the module configs of config/module/relay_imitation_learning.yaml, and the fixture names."""
import numpy as np
import torch

from tacorl_amd import synth

GOLDENS = ("ril", "ril_twocam")
ROLES = ("obs", "low_level_goal", "high_level_goal", "high_level_action")
TARGET = "tacorl_amd.modules.relay_imitation_learning.relay_imitation_learning.RelayImitationLearning"
P = "tacorl.networks."


def make_ril_batch(seed, B, cams_hw):
    """RelayImitationLearningDataset batch (reference datamodule/dataset/relay_imitation_learning_dataset.py:100-107):
    obs / low_level_goal / high_level_goal / high_level_action as dicts camera -> (B,3,H,W) in [-1,1], low_level_action (B,7)
    with a +-1 gripper column."""
    rs = synth._rs(seed, "ril")
    cams = sorted(cams_hw.items())
    batch = {role: {c: synth._img(rs, B, 3, h, w) for c, (h, w) in cams} for role in ROLES}
    batch["low_level_action"] = synth._actions(rs, B)
    return batch


def to_uint8_hwc(batch):
    """The same batch as the dataset's raw uint8 HWC frames would give it after ToTensor + Normalize(0.5, 0.5): returns
    (uint8 batch, the fp32 NCHW batch those frames normalise to)."""
    u8, f32 = {}, {}
    for role in ROLES:
        u8[role], f32[role] = {}, {}
        for c, t in batch[role].items():
            q = ((t * 0.5 + 0.5) * 255.0).round().clamp(0, 255).to(torch.uint8)
            u8[role][c] = q.permute(0, 2, 3, 1).contiguous()
            f32[role][c] = (q.float() / 255.0 - 0.5) / 0.5
    u8["low_level_action"] = f32["low_level_action"] = batch["low_level_action"]
    return u8, f32


def enc_cfg():
    return {"_target_": P + "visual_encoders.encoder.LMPVisionEncoder", "latent_dim": 32, "hidden_dim": 256,
            "normalize_output": False}


def ril_cfg(low=("rgb_static",), high=None, num_layers=4, hidden_dim=1024, lr=1e-4, last_layer_activation="Tanh", **kw):
    """Constructor keywords of the module as config/module/relay_imitation_learning.yaml composes them."""
    high = list(low if high is None else high)
    low = list(low)

    def actor(dg, action_dim):
        c = {"_target_": P + "actor_critic.actor.Actor", "_recursive_": False, "action_dim": action_dim,
             "policy": {"_target_": P + "actor_critic.actor.MLPPolicy", "num_layers": num_layers, "hidden_dim": hidden_dim}}
        if dg:
            c["discrete_gripper"] = True
        return c

    cfg = dict(
        env={},
        goal_encoder={"_target_": P + "visual_encoders.goal_encoder.VisualGoalEncoder", "in_features": None, "out_features": 32,
                      "hidden_size": 256, "activation_function": "ReLU", "last_layer_activation": last_layer_activation},
        perceptual_encoder={"_target_": P + "representation.representation_network.LateFusion", "_recursive_": False,
                            "networks": {"rgb_static": enc_cfg(), "rgb_gripper": enc_cfg()}},
        high_level_policy=actor(False, 32), low_level_policy=actor(True, 7),
        high_level_policy_modalities=high, low_level_policy_modalities=low, lr=lr)
    cfg.update(kw)
    return cfg


def cfg_of_golden(g, **kw):
    c = g.cfg
    return ril_cfg(low=c["low"], high=c["high"], num_layers=c["num_layers"], hidden_dim=c["hidden_dim"], lr=c["lr"], **kw)


def golden_batch(g, step):
    return make_ril_batch(g.cfg["seed"] * 100 + step, g.cfg["B"], g.cams)


def rel_err(got, exp):
    exp = np.asarray(exp, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - exp)) / max(np.max(np.abs(exp)), 1e-30))
