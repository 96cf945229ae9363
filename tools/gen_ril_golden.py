"""Generate tests/golden/ril.npz and tests/golden/ril_twocam.npz by running the UNMODIFIED reference
RelayImitationLearning module on CPU (needs the reference checkout that oracle/ref_harness.py points at).

    python tools/gen_ril_golden.py            # both cases
    python tools/gen_ril_golden.py ril        # one case

Format: oracle/gen_golden.py's (config + seed, logged scalars per step, fingerprints - synth.tensor_stats - of every
gradient and of every parameter after the step, parameter names and shapes).  Parameters and batches are re-derived from the
seed (tacorl_amd.synth / tests.ril_util), so a fixture holds no image, no weight and no reference source text.  The
reference constructor calls make_env(env); the name is replaced in the imported module's namespace by a function that
returns None (the simulator is not part of the step)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as H  # noqa: E402
from oracle.gen_golden import OUT, _stats_dict  # noqa: E402
from tacorl_amd import synth  # noqa: E402
from tests import ril_util as U  # noqa: E402

# config/module/relay_imitation_learning.yaml: 4 x 1024 policies, Tanh goal encoder, lr 1e-4
YAML = dict(num_layers=4, hidden_dim=1024, lr=1e-4)
CASES = {
    "ril": dict(kind="ril", B=3, cams={"rgb_static": (84, 84)}, low=["rgb_static"], high=["rgb_static"], steps=2, seed=51,
                **YAML),
    # the two policies read the cameras in opposite orders: a swapped concatenation or camera index cannot pass
    "ril_twocam": dict(kind="ril", B=3, cams={"rgb_static": (84, 84), "rgb_gripper": (64, 64)},
                       low=["rgb_static", "rgb_gripper"], high=["rgb_gripper", "rgb_static"], steps=2, seed=52, **YAML),
}


def build(c):
    H.install_shims()
    import tacorl.modules.relay_imitation_learning.relay_imitation_learning as R

    R.make_env = lambda *a, **k: None
    kw = U.ril_cfg(low=c["low"], high=c["high"], num_layers=c["num_layers"], hidden_dim=c["hidden_dim"], lr=c["lr"])
    kw["env"] = None
    return R.RelayImitationLearning(**kw)


def run_case(name, c):
    torch.manual_seed(c["seed"])
    torch.set_num_threads(8)
    mod = build(c)
    synth.fill_params_(mod, c["seed"])
    mod.train()
    out = {"param_names": np.array([n for n, _ in mod.named_parameters()]),
           "param_shapes": np.array(json.dumps([list(p.shape) for _, p in mod.named_parameters()])),
           "param_requires_grad": np.array([p.requires_grad for _, p in mod.named_parameters()])}
    opt = mod.optimizers()[0]
    for step in range(c["steps"]):
        batch = U.make_ril_batch(c["seed"] * 100 + step, c["B"], c["cams"])
        tape = H.NoiseTape()
        mod.logged, mod.grad_log = {}, []
        with H.record_noise(tape):
            loss = mod.training_step(batch, 0)
            opt.zero_grad()
            mod.manual_backward(loss)
            opt.step()
        assert not tape.draws, "the RIL step draws no random numbers"
        out[f"s{step}/logged"] = np.array(json.dumps(mod.logged))
        _stats_dict(f"s{step}/grad", mod.grad_log[0].items(), out)
        _stats_dict(f"s{step}/param", mod.named_parameters(), out)
        print(f"[{name}] step {step}: " + ", ".join(f"{k}={v:.6g}" for k, v in sorted(mod.logged.items())))
    out["config"] = np.array(json.dumps(dict(c)))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"[{name}] wrote {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    for n in sys.argv[1:] or list(CASES):
        run_case(n, CASES[n])
