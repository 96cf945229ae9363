"""Generate tests/golden/cql_goalcams.npz by running the UNMODIFIED reference on CPU: CQL_Offline with goal cameras
that differ from the observation cameras (config/experiment/cql_gripper_real_world.yaml: the goal is a third-person
image, the wrist camera only informs the current state).

Run in the build container only (needs the reference checkout):
    python oracle/gen_goalcams_golden.py

ref_harness.build_cql builds the symmetric module (goal_modalities = obs_modalities), so the module is constructed here
from the same sub-configs.  The fixture has the format of gen_golden.run_case (config + seed, noise tape, logged
scalars, gradient and parameter fingerprints; no reference source text); its config also records `obs_cams` and
`goal_cams`, the two ordered modality lists.  The two camera geometries differ so that a swapped camera index
cannot pass.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import gen_golden as G  # noqa: E402
from oracle import ref_harness as H  # noqa: E402
from tacorl_amd import synth  # noqa: E402

NAME = "cql_goalcams"
CASE = dict(kind="cql", B=3, cams={"rgb_static": (84, 84), "rgb_gripper": (64, 64)}, epoch=5, steps=2, seed=51,
            obs_cams=["rgb_static", "rgb_gripper"], goal_cams=["rgb_static"], overrides=dict(n_action_samples=4))


def build(c):
    H.install_shims()
    from tacorl.modules.cql.cql_offline_lightning import CQL_Offline

    kw = dict(H.CQL_YAML)
    kw.update(c.get("overrides", {}))
    return CQL_Offline(actor=H.actor_cfg(discrete_gripper=True), critic=H.critic_cfg(), actor_encoder=H.rep_cfg(),
                       critic_encoder=H.rep_cfg(), goal_encoder=H.goal_cfg(), real_world=True,
                       obs_modalities=list(c["obs_cams"]), goal_modalities=list(c["goal_cams"]), action_dim=7, **kw)


def run(name=NAME, c=CASE):
    torch.manual_seed(c["seed"])
    torch.set_num_threads(8)
    mod = build(c)
    synth.fill_params_(mod, c["seed"])
    mod.train()
    mod.current_epoch = c["epoch"]
    out = {"param_names": np.array([n for n, _ in mod.named_parameters()]),
           "param_shapes": np.array(json.dumps([list(p.shape) for _, p in mod.named_parameters()])),
           "param_requires_grad": np.array([p.requires_grad for _, p in mod.named_parameters()])}
    order = ["log_alpha", "log_alpha_prime", "actor", "q1", "q2"]
    for step in range(c["steps"]):
        batch = synth.make_transition_batch(c["seed"] * 100 + step, c["B"], c["cams"])
        tape = H.NoiseTape()
        mod.logged, mod.grad_log = {}, []
        with H.record_noise(tape):
            mod.training_step(batch, 0)
        for i, (kind, t) in enumerate(tape.draws):
            out[f"s{step}/noise/{i:02d}_{kind}"] = t.numpy()
        out[f"s{step}/logged"] = np.array(json.dumps(mod.logged))
        assert len(mod.grad_log) == len(order), (len(mod.grad_log), order)
        for g, gl in zip(order, mod.grad_log):
            G._stats_dict(f"s{step}/grad", [(n, t) for n, t in gl.items() if G._group_of(n) == g], out)
        G._stats_dict(f"s{step}/param", mod.named_parameters(), out)
        print(f"[{name}] step {step}: " + ", ".join(f"{k.split('/')[-1]}={v:.5g}" for k, v in sorted(mod.logged.items())))
    out["config"] = np.array(json.dumps(dict(c)))
    os.makedirs(G.OUT, exist_ok=True)
    path = os.path.join(G.OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"[{name}] wrote {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    run()
