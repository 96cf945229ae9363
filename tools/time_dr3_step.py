"""What the DR3 term costs per training step: the headline TACORL shape (bench.py's default: B = 256, window 16, one 84 x 84
camera, bf16, hipGraph) and C5 (CQL_Offline, 32 action samples, B = 1024), each with the term off and on, on one GPU.

    python tools/time_dr3_step.py [--steps 300] [--warmup 30] [--rounds 3] [--only off]

bench.py's conventions, read only: its module and batch builders (build_module / synth_batch, time_other_configs' C5), the
captured graph, metrics read back every 50 steps, warm-up steps first; then per-step device times from a HIP event after
every step, and their median.  "off" and "on" are timed in alternating blocks (`--rounds` of `--steps` steps each) in one
process, so that clock drift falls on both.  `--only off` times the unchanged path alone: the same command on the commit
before the term existed gives the pair the documents compare.  Prints one JSON line per configuration."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

DR3 = dict(with_dr3=True, dr3_coefficient=0.03)  # the reference default (config/module/tacorl.yaml)


def headline(dev, dtype, dr3):
    if dr3:  # build_module takes no module options: the same construction with the term switched on
        import unittest.mock as um

        from tacorl_amd.modules.tacorl import tacorl as T

        real = T.TACORL
        with um.patch.object(T, "TACORL", lambda **kw: real(**kw, **DR3)):
            mod = bench.build_module(dev, dtype, 16, 1)
        assert mod.engine.dr3 == DR3["dr3_coefficient"]
    else:
        mod = bench.build_module(dev, dtype, 16, 1)
    return mod, bench.synth_batch(256, 16, 84, 84, dev, bench.DATA_SEED), (), 256


def c5(dev, dtype, dr3):
    from tacorl_amd import synth
    from tacorl_amd.modules.cql.cql_offline_lightning import CQL_Offline

    actor = {"policy": {"num_layers": 3, "hidden_dim": 256}, "discrete_gripper": True}
    critic = {"q_network": {"num_layers": 3, "hidden_dim": 256, "last_layer_activation": "Identity"}}
    torch.manual_seed(bench.PARAM_SEED)
    mod = CQL_Offline(actor=actor, critic=critic, real_world=True, obs_modalities=["rgb_static"], goal_modalities=["rgb_static"],
                      action_dim=7, device=dev, compute_dtype=dtype, image_dtype=dtype, discount=0.99, actor_lr=1e-4,
                      critic_lr=3e-4, conservative_weight=1.0, n_action_samples=32, with_lagrange=True, reward_scale=10.0,
                      deterministic_backup=False, bc_epochs=5, **(DR3 if dr3 else {}))
    mod.current_epoch = 5
    to_dev = lambda x: {k: to_dev(v) for k, v in x.items()} if isinstance(x, dict) else (x.to(dev) if torch.is_tensor(x) else x)  # noqa: E731
    return mod, to_dev(synth.make_transition_batch(7, 1024, {"rgb_static": (84, 84)})), (0,), 1024


def block(mod, batch, args, steps):
    """Per-step device times (ms) of `steps` training steps."""
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    evs[0].record()
    for i in range(steps):
        mod.training_step(batch, *args)
        evs[i + 1].record()
    torch.cuda.synchronize()
    return [evs[i].elapsed_time(evs[i + 1]) for i in range(steps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--only", default=None, choices=["off"], help="time the path without the term alone")
    a = ap.parse_args()
    dev = "cuda:0"
    for name, make in (("headline_tacorl_b256", headline), ("c5_cql_n32_b1024", c5)):
        modes = ["off"] if a.only else ["off", "on"]
        built = {}
        for m in modes:
            mod, batch, args, B = make(dev, a.dtype, m == "on")
            mod.enable_graph()
            mod.log_every_n_steps = 50
            for _ in range(a.warmup):
                mod.training_step(batch, *args)
            torch.cuda.synchronize()
            built[m] = (mod, batch, args)
        ts = {m: [] for m in modes}
        for _ in range(a.rounds):
            for m in modes:
                ts[m] += block(*built[m], a.steps)
        res = {"config": name, "dtype": a.dtype, "batch": B, "steps_per_mode": a.rounds * a.steps, "warmup": a.warmup}
        for m in modes:
            s = sorted(ts[m])
            res[f"dr3_{m}_median_ms"] = round(s[len(s) // 2], 4)
            res[f"dr3_{m}_p10_ms"], res[f"dr3_{m}_p90_ms"] = round(s[len(s) // 10], 4), round(s[len(s) * 9 // 10], 4)
            eng = built[m][0].engine
            res[f"dr3_{m}_encoder_images"] = sum(x[4] for c in eng.enc_cams for x in eng._all_problems(c))
            res[f"dr3_{m}_losses_finite"] = bool(torch.isfinite(eng.logs).all().item())
        if "on" in ts:
            res["on_over_off"] = round(res["dr3_on_median_ms"] / res["dr3_off_median_ms"], 4)
        print(json.dumps(res), flush=True)
        for m in modes:
            built[m][0]._graphs = {}
        del built
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
