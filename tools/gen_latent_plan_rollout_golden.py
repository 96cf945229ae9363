"""Generate tests/golden/{rollout_playlmp,rollout_d4rl}.npz by running the UNMODIFIED reference classes on CPU through the call
sequence of its latent-plan rollout managers (evaluation/rollout_manager.py:232-260 LatentPlanRollout; evaluation/
rollout_manager_d4rl.py:137-146, :206-229), batched: needs the reference checkout that oracle/ref_harness.py points at.

    python tools/gen_latent_plan_rollout_golden.py                   # both
    python tools/gen_latent_plan_rollout_golden.py rollout_d4rl      # one

rollout_playlmp: the image PlayLMP, one camera 84 x 84, n = 2.  rollout_d4rl: the D4RL PlayLMP and the TACORL built on it,
n = 3.  Each records `plan_proposal.get_dist(...)`'s normal_mean / normal_std, one `sample()` with its draw, three
`action_decoder.act` steps with their draws from a cleared hidden state, and the final hidden state; rollout_d4rl also
the TACORL actor's deterministic plan, which its act steps decode (rollout_playlmp decodes the sampled plan).  Format:
oracle/gen_golden.py's rollout goldens - parameters and batches are re-derived from the seed (tacorl_amd.synth), so a
fixture holds no weight and no reference source text."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as H  # noqa: E402
from oracle.gen_golden import OUT  # noqa: E402
from tacorl_amd import synth  # noqa: E402

CASES = {
    "rollout_playlmp": dict(kind="rollout_playlmp", B=2, T=4, cams={"rgb_static": (84, 84)}, latent=16, seed=23),
    "rollout_d4rl": dict(kind="rollout_d4rl", B=3, T=8, cams={}, latent=16, seed=66, env="antmaze-large-diverse-v0",
                         finetune_ad=False),
}
STEPS = 3


def _decode(action_decoder, plan, emb_of_step, out):
    action_decoder.clear_hidden_state()
    acts = []
    for t in range(STEPS):
        acts.append(action_decoder.act(latent_plan=plan, perceptual_emb=emb_of_step(t).unsqueeze(1)).clone())
    out.update(actions=torch.stack(acts).numpy(), hidden=action_decoder.hidden_state.numpy())


def run_playlmp(c, out, tape):
    names = tuple(sorted(c["cams"]))
    mod = H.build_play_lmp(cams=names, latent_plan_dim=c["latent"], seq_len=16)
    synth.fill_params_(mod, c["seed"])
    mod.eval()
    batch = synth.make_play_batch(c["seed"] * 100, c["B"], c["T"], c["cams"])
    frame = lambda t: {k: v[:, t] for k, v in batch["states"].items()}  # noqa: E731
    pe = mod.perceptual_encoder
    with torch.no_grad(), H.record_noise(tape):
        emb_state = pe.get_state_from_observation(observation=frame(0), modalities=list(names), cat_output=False)
        assert isinstance(emb_state, dict) and sorted(emb_state) == list(names)
        pp_state = torch.cat([emb_state[k] for k in mod.plan_proposal_obs_modalities], dim=-1)
        pp_goal_in = pe.get_state_from_observation(observation=batch["goal"], modalities=mod.plan_proposal_goal_modalities)
        pp_goal = mod.goal_encoder(pp_goal_in)
        dist = mod.plan_proposal.get_dist(state_emb=pp_state, goal_emb=pp_goal)
        plan = dist.sample()
        embs = [pe.get_state_from_observation(observation=frame(t), modalities=mod.action_decoder_modalities) for t in range(STEPS)]
        _decode(mod.action_decoder, plan, lambda t: embs[t], out)
    out.update(pp_state=pp_state.numpy(), pp_goal=pp_goal.numpy(), normal_mean=dist.normal_mean.numpy(),
               normal_std=dist.normal_std.numpy(), plan_sampled=plan.numpy(), ad_state=torch.stack(embs).numpy())
    return mod


def run_d4rl(c, out, tape):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_d4rl_golden as D

    lmp = D.build_play_lmp(c)
    mod = D.build_tacorl(c, lmp)
    synth.fill_params_(mod, c["seed"])
    mod.eval()
    batch = synth.make_d4rl_window_batch(c["seed"] * 100, c["B"], c["T"], D.STATE_DIM, D.ACTION_DIM)
    obs, goal = batch["observations"], batch["goal"]
    with torch.no_grad(), H.record_noise(tape):
        dist = lmp.plan_proposal.get_dist(state_emb=obs[:, 0], goal_emb=goal)
        plan_s = dist.sample()
        plan, lp = mod.actor.get_actions(torch.cat([obs[:, 0], goal], dim=-1), deterministic=True, reparameterize=False)
        assert float(lp.abs().max()) == 0.0
        _decode(mod.action_decoder, plan, lambda t: obs[:, t], out)
    out.update(normal_mean=dist.normal_mean.numpy(), normal_std=dist.normal_std.numpy(), plan_sampled=plan_s.numpy(),
               plan=plan.numpy())
    return mod


def run_case(name, c):
    torch.manual_seed(c["seed"])
    torch.set_num_threads(8)
    out, tape = {}, H.NoiseTape()
    mod = (run_playlmp if c["kind"] == "rollout_playlmp" else run_d4rl)(c, out, tape)
    kinds = [k for k, _ in tape.draws]
    assert len(kinds) == 1 + 2 * STEPS and kinds[0] == "normal", kinds  # the plan's draw, then two uniform draws per act
    for i, (kind, t) in enumerate(tape.draws):
        out[f"s0/noise/{i:02d}_{kind}"] = t.numpy()
    out["param_names"] = np.array([n for n, _ in mod.named_parameters()])
    out["param_shapes"] = np.array(json.dumps([list(p.shape) for _, p in mod.named_parameters()]))
    out["param_requires_grad"] = np.array([p.requires_grad for _, p in mod.named_parameters()])
    out["config"] = np.array(json.dumps(dict(c)))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"[{name}] wrote {os.path.getsize(path) / 1e3:.1f} kB; draws: {kinds}; " +
          ", ".join(f"{k}{tuple(v.shape)}" for k, v in out.items() if isinstance(v, np.ndarray) and v.ndim and "/" not in k
                    and not k.startswith("param")))


if __name__ == "__main__":
    for n in sys.argv[1:] or list(CASES):
        run_case(n, CASES[n])
