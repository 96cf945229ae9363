"""Generate tests/golden/rollout_ril.npz by running the UNMODIFIED reference RelayImitationLearning module on CPU through the
call sequence of its rollout manager (evaluation/rollout_manager.py:480-510), batched: needs the reference checkout that
oracle/ref_harness.py points at.

    python tools/gen_ril_rollout_golden.py

The case is ril_twocam's configuration (tools/gen_ril_golden.py: cameras 84 x 84 and 64 x 64, the two policies read them in
opposite orders, 4 x 1024 policies), n = 3 rows, 3 steps, eval mode, no_grad.  Recorded: per step the per-camera state
embeddings; once the goal's per-camera embeddings, the goal-encoder input and output, the high-level head's normal_mean and
the sub-goal; per step the low-level head's mean and gripper logits and the (3, 7) action.  Format:
tools/gen_latent_plan_rollout_golden.py's - parameters and images are re-derived from the seed (tacorl_amd.synth /
tests.ril_util), so the fixture holds no weight and no reference source text.

Gap condition: a fixture in which any recorded gripper decision has |l1 - l0| < GAP * max(|l0|, |l1|) is refused (GAP = 1e-2,
100 x the parity tolerance of 1e-4: no implementation inside the tolerance can decide the other way).  Seeds are tried upward
from 52 and the one kept is recorded in the config."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle.gen_golden import OUT  # noqa: E402
from tacorl_amd import synth  # noqa: E402
from tests import ril_util as U  # noqa: E402
import gen_ril_golden as G  # noqa: E402

NAME = "rollout_ril"
STEPS, GAP, FIRST_SEED, MAX_TRIES = 3, 1e-2, 52, 32
CASE = dict(G.CASES["ril_twocam"], kind="rollout_ril", steps=STEPS)


def gap_ok(logits):
    """logits (..., 2): every decision's |l1 - l0| >= GAP * max(|l0|, |l1|)."""
    l0, l1 = logits[..., 0], logits[..., 1]
    return bool(np.all(np.abs(l1 - l0) >= GAP * np.maximum(np.abs(l0), np.abs(l1))))


def frames(c):
    """(observation images per step, goal images): the `obs` role of batch seed * 100 + t, the `high_level_goal` role of
    batch seed * 100."""
    batches = [U.make_ril_batch(c["seed"] * 100 + t, c["B"], c["cams"]) for t in range(c["steps"])]
    return [b["obs"] for b in batches], batches[0]["high_level_goal"]


def run(c):
    torch.manual_seed(c["seed"])
    torch.set_num_threads(8)
    mod = G.build(c)
    synth.fill_params_(mod, c["seed"])
    mod.eval()
    obs, goal = frames(c)
    pe, cams = mod.perceptual_encoder, sorted(c["cams"])
    out = {}
    with torch.no_grad():
        # rollout_manager.py:481-499, once (the three steps lie inside one plan_duration)
        emb0 = pe.get_state_from_observation(observation=obs[0], modalities=mod.all_modalities, cat_output=False)
        state_h = torch.cat([emb0[k] for k in mod.high_level_policy_modalities], dim=-1)
        goal_d = pe.get_state_from_observation(observation=goal, modalities=mod.high_level_policy_modalities, cat_output=False)
        goal_in = pe.get_state_from_observation(observation=goal, modalities=mod.high_level_policy_modalities)
        goal_out = mod.goal_encoder(goal_in)
        high_obs = torch.cat([state_h, goal_out], dim=-1)
        high_mean = mod.high_level_policy.get_dist(high_obs).normal_mean
        subgoal, _ = mod.high_level_policy.get_actions(high_obs, deterministic=True)
        embs, means, logits, actions = {k: [] for k in cams}, [], [], []
        for t in range(c["steps"]):  # :501-510
            d = pe.get_state_from_observation(observation=obs[t], modalities=mod.all_modalities, cat_output=False)
            for k in cams:
                embs[k].append(d[k])
            state_l = pe.get_state_from_observation(observation=obs[t], modalities=mod.low_level_policy_modalities)
            low_obs = torch.cat([state_l, subgoal], dim=-1)
            mean, _, lg = mod.low_level_policy(low_obs)
            action, _ = mod.low_level_policy.get_actions(low_obs, deterministic=True)
            means.append(mean), logits.append(lg), actions.append(action)
    for k in cams:
        out[f"emb/{k}"] = torch.stack(embs[k]).numpy()
        out[f"goal_emb/{k}"] = goal_d[k].numpy()
    out.update(goal_in=goal_in.numpy(), goal_out=goal_out.numpy(), high_mean=high_mean.numpy(), subgoal=subgoal.numpy(),
               low_mean=torch.stack(means).numpy(), low_logits=torch.stack(logits).numpy(), actions=torch.stack(actions).numpy())
    out["param_names"] = np.array([n for n, _ in mod.named_parameters()])
    out["param_shapes"] = np.array(json.dumps([list(p.shape) for _, p in mod.named_parameters()]))
    out["param_requires_grad"] = np.array([p.requires_grad for _, p in mod.named_parameters()])
    out["config"] = np.array(json.dumps(dict(c)))
    return out


if __name__ == "__main__":
    for seed in range(FIRST_SEED, FIRST_SEED + MAX_TRIES):
        out = run(dict(CASE, seed=seed))
        if gap_ok(out["low_logits"]):
            break
        print(f"[{NAME}] seed {seed}: a gripper decision is closer than {GAP} relative - refused")
    else:
        raise SystemExit(f"no seed in {FIRST_SEED} .. {FIRST_SEED + MAX_TRIES - 1} meets the gap condition: nothing written")
    path = os.path.join(OUT, NAME + ".npz")
    np.savez_compressed(path, **out)
    lg = out["low_logits"]
    print(f"[{NAME}] seed {seed}: wrote {os.path.getsize(path) / 1e3:.1f} kB; smallest relative logit gap "
          f"{np.min(np.abs(lg[..., 1] - lg[..., 0]) / np.maximum(np.abs(lg[..., 0]), np.abs(lg[..., 1]))):.3g}; actions "
          f"{out['actions'].shape}, gripper column {out['actions'][..., -1].tolist()}")
