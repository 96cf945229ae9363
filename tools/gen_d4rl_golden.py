"""Generate tests/golden/{playlmp_d4rl,tacorl_d4rl_q,tacorl_d4rl_ad,val_tacorl_d4rl}.npz by running the UNMODIFIED reference
D4RL modules (modules/play_lmp/play_lmp_d4rl.py, modules/tacorl/tacorl_d4rl.py) on CPU (needs the reference checkout that
oracle/ref_harness.py points at).

    python tools/gen_d4rl_golden.py                  # all cases
    python tools/gen_d4rl_golden.py tacorl_d4rl_q    # one case
    python tools/gen_d4rl_golden.py --time           # no fixture: the reference's CPU step time at the shapes
                                                     # tools/time_d4rl_step.py times on the GPU (profiles/d4rl_step.md)

Format: oracle/gen_golden.py's - config + seed, the noise tape, logged scalars per step, the sampled latent plan, fingerprints
(synth.tensor_stats) of every gradient as its optimiser saw it and of every parameter after the step, parameter names and shapes.
Parameters and batches are re-derived from the seed (tacorl_amd.synth), so a fixture holds no weight and no reference source
text.  Beside oracle.ref_harness's stand-ins this adds two of its own before the reference modules are imported: an empty
`d4rl` module and a `gym.make` whose result has the AntMaze spaces (observation (29,), action (8,) in [-1, 1]) - the only
facts the modules read from the environment.  TACORL's `load_pl_module_from_checkpoint` is replaced in the imported module's
namespace by a function that returns the PlayLMP built here.

The reference's D4RL TACORL inherits `validation_step` from its flat CQL parent, which expects a transition batch and cannot
take the window batch the module trains on.  val_tacorl_d4rl therefore records the sequence the image TACORL's validation_step
runs (reference modules/tacorl/tacorl.py:275-287) through the D4RL module's own methods: get_pr_latent_plan,
compute_action_decoder_update(optimize=False), get_rl_batch, compute_update(optimize=False), in eval mode under no_grad."""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as H  # noqa: E402
from oracle.gen_golden import OUT, _group_of, _stats_dict  # noqa: E402
from tacorl_amd import synth  # noqa: E402

STATE_DIM, ACTION_DIM = 29, 8
# config/experiment/{play_lmp,tacorl}_d4rl.yaml: window min = max = 8, latent plan 16; config/module/tacorl_d4rl.yaml
BASE = dict(B=3, T=8, latent=16, cams={}, steps=2, env="antmaze-large-diverse-v0")
TACORL_YAML = dict(action_decoder_lr=3e-4, actor_lr=1e-4, critic_lr=3e-4, discount=0.95, conservative_weight=1.0,
                   reward_scale=10.0, n_action_samples=4, with_lagrange=True, deterministic_backup=True, bc_epochs=0,
                   with_vib=False, vib_coefficient=0.03)
CASES = {
    # the seq-VAE step as the reference trains it: plan-recognition dropout 0.1 in train mode (transformer.yaml:9)
    "playlmp_d4rl": dict(BASE, kind="playlmp_d4rl", seed=61, dropout_p=0.1),
    "tacorl_d4rl_q": dict(BASE, kind="tacorl_d4rl", seed=62, finetune_ad=False),
    "tacorl_d4rl_ad": dict(BASE, kind="tacorl_d4rl", seed=63, finetune_ad=True),
    "val_tacorl_d4rl": dict(BASE, kind="tacorl_d4rl", seed=64, finetune_ad=True, steps=1, validate=True),
}


class _Space:
    def __init__(self, n):
        self.shape = (n,)
        self.high, self.low = np.ones(n, dtype=np.float32), -np.ones(n, dtype=np.float32)


def install_d4rl_shims():
    H.install_shims()
    sys.modules.setdefault("d4rl", types.ModuleType("d4rl"))
    env = types.SimpleNamespace(observation_space=_Space(STATE_DIM), action_space=_Space(ACTION_DIM))
    sys.modules["gym"].make = lambda name, *a, **k: env


def build_play_lmp(c):
    install_d4rl_shims()
    from tacorl.modules.play_lmp.play_lmp_d4rl import PlayLMP

    ad = dict(H.ad_cfg(c["latent"]), discrete_gripper=False)  # config/module/play_lmp_d4rl.yaml:11-12
    return PlayLMP(plan_proposal=H.actor_cfg(), plan_recognition=H.pr_cfg(c["latent"], c["T"], c.get("dropout_p", 0.0)),
                   action_decoder=ad, lr=1e-4, kl_beta=1e-3, d4rl_env=c["env"])


def build_tacorl(c, lmp):
    import tacorl.modules.tacorl.tacorl_d4rl as T

    T.load_pl_module_from_checkpoint = lambda *a, **k: lmp
    return T.TACORL(play_lmp_dir="/nonexistent", finetune_action_decoder=c["finetune_ad"], critic=H.critic_cfg(),
                    d4rl_env=c["env"], **TACORL_YAML)


def run_case(name, c):
    torch.manual_seed(c["seed"])
    torch.set_num_threads(8)
    lmp = build_play_lmp(c)
    mod = build_tacorl(c, lmp) if c["kind"] == "tacorl_d4rl" else lmp
    synth.fill_params_(mod, c["seed"])
    mod.train()
    if c.get("validate"):
        mod.eval()
    out = {"param_names": np.array([n for n, _ in mod.named_parameters()]),
           "param_shapes": np.array(json.dumps([list(p.shape) for _, p in mod.named_parameters()])),
           "param_requires_grad": np.array([p.requires_grad for _, p in mod.named_parameters()])}
    for step in range(c["steps"]):
        batch = synth.make_d4rl_window_batch(c["seed"] * 100 + step, c["B"], c["T"], STATE_DIM, ACTION_DIM)
        assert batch["goal_reached"].any() and not batch["goal_reached"].all()
        tape = H.NoiseTape()
        mod.logged, mod.grad_log = {}, []
        if c["kind"] == "playlmp_d4rl":
            opt = mod.optimizers()[0]
            with H.record_noise(tape):
                loss = mod.training_step(batch, 0)
                opt.zero_grad()
                mod.manual_backward(loss)
                opt.step()
            _stats_dict(f"s{step}/grad", mod.grad_log[0].items(), out)
        elif c.get("validate"):
            before = {n: p.detach().clone() for n, p in mod.named_parameters()}
            with torch.no_grad(), H.record_noise(tape):
                plan = mod.get_pr_latent_plan(batch)
                mod.compute_action_decoder_update(states=batch["observations"], actions=batch["actions"], latent_plan=plan,
                                                  optimize=False, log_type="validation")
                mod.compute_update(mod.get_rl_batch(batch, plan), optimize=False, log_type="validation")
            assert all(torch.equal(before[n], p) for n, p in mod.named_parameters()), "the validation pass moved a parameter"
            out[f"s{step}/latent_plan"] = plan.detach().numpy()
        else:
            orig, cap = mod.get_pr_latent_plan, {}

            def wrapped(b, _o=orig, _c=cap):
                _c["plan"] = _o(b).detach().clone()
                return _c["plan"]

            mod.get_pr_latent_plan = wrapped
            with H.record_noise(tape):
                mod.training_step(batch)
            mod.get_pr_latent_plan = orig
            out[f"s{step}/latent_plan"] = cap["plan"].numpy()
            # grads as each optimiser saw them: one manual_backward per optimiser, in the step's order
            order = (["action_decoder"] if c["finetune_ad"] else []) + ["log_alpha", "log_alpha_prime", "actor", "q1", "q2"]
            assert len(mod.grad_log) == len(order), (len(mod.grad_log), order)
            for g, gl in zip(order, mod.grad_log):
                _stats_dict(f"s{step}/grad", [(n, t) for n, t in gl.items() if _group_of(n) == g], out)
        for i, (kind, t) in enumerate(tape.draws):
            out[f"s{step}/noise/{i:02d}_{kind}"] = t.numpy()
        out[f"s{step}/logged"] = np.array(json.dumps(mod.logged))
        if not c.get("validate"):
            _stats_dict(f"s{step}/param", mod.named_parameters(), out)
        print(f"[{name}] step {step}: " + ", ".join(f"{k.split('/')[-1]}={v:.5g}" for k, v in sorted(mod.logged.items())))
        print(f"[{name}] draws: {[k for k, _ in tape.draws]}")
    out["config"] = np.array(json.dumps(dict(c)))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"[{name}] wrote {os.path.getsize(path) / 1e3:.1f} kB")


def time_reference(steps=5):
    """`--time`: the reference's own CPU step time at the shapes tools/time_d4rl_step.py times on the GPU (fp32, torch's
    default thread count, best of `steps` steps after one warm-up) - a reported baseline, not a target."""
    import time

    res = {"threads": torch.get_num_threads()}
    for name, kind, B in (("tacorl_b64", "tacorl_d4rl", 64), ("tacorl_b256", "tacorl_d4rl", 256), ("playlmp_b64", "playlmp_d4rl", 64)):
        c = dict(BASE, kind=kind, B=B, seed=7, finetune_ad=True, dropout_p=0.1)
        lmp = build_play_lmp(c)
        mod = build_tacorl(c, lmp) if kind == "tacorl_d4rl" else lmp
        synth.fill_params_(mod, c["seed"])
        mod.train()
        batch = synth.make_d4rl_window_batch(7, B, c["T"], STATE_DIM, ACTION_DIM)
        ts = []
        for _ in range(steps + 1):
            t0 = time.perf_counter()
            if kind == "playlmp_d4rl":
                opt = mod.optimizers()[0]
                loss = mod.training_step(batch, 0)
                opt.zero_grad()
                loss.backward()
                opt.step()
            else:
                mod.grad_log = []
                mod.training_step(batch)
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name] = {"best_ms": round(min(ts[1:]), 1), "median_ms": round(sorted(ts[1:])[len(ts[1:]) // 2], 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    if sys.argv[1:] == ["--time"]:
        time_reference()
    else:
        for n in sys.argv[1:] or list(CASES):
            run_case(n, CASES[n])
