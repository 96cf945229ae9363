"""Time CQL_Offline at BASELINE config C5 (B = 1024, 32 action samples, 84x84, bf16, hipGraph on, metrics read back every
50 steps - bench.py's conventions for its `c5_cql_n32_b1024` line) fed four ways, on one GPU:

  (a) the step on a resident batch (the same tensors every step);
  (b) the step fed by HbmTransitionReplay.batch(fused=True) with fresh device draws per step, without and with the
      train-time augmentation;
  (c) the sampler alone: HbmTransitionReplay.batch() = one tacorl_sample_transitions launch, device events around
      back-to-back calls (an upper bound on the kernel: the calls are paced by the host), and the device draws;
  (d) the host sampler, TransitionIndex.sample, for the same B (host clock).

    python tools/time_transition_replay.py [--steps 400] [--frames 40000] [--out FILE]

Prints one JSON line (and writes it to --out).  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=40000)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_transition_replay: needs a GPU")
    from tacorl_amd import _lib, synth
    from tacorl_amd.data.augment import AugmentSpec, draw_transition_batch_augmentation
    from tacorl_amd.data.replay import HbmTransitionReplay, TransitionIndex
    from tacorl_amd.modules.cql.cql_offline_lightning import CQL_Offline

    dev, B, N = "cuda:0", a.batch, a.frames
    _lib.call("tacorl_hip_init", 0)

    def module():
        torch.manual_seed(0)
        m = CQL_Offline(actor={"policy": {"num_layers": 3, "hidden_dim": 256}, "discrete_gripper": True},
                        critic={"q_network": {"num_layers": 3, "hidden_dim": 256, "last_layer_activation": "Identity"}},
                        real_world=True, obs_modalities=["rgb_static"], goal_modalities=["rgb_static"], action_dim=7, device=dev,
                        compute_dtype=a.dtype, image_dtype=a.dtype, discount=0.99, actor_lr=1e-4, critic_lr=3e-4,
                        conservative_weight=1.0, n_action_samples=32, with_lagrange=True, reward_scale=10.0,
                        deterministic_backup=False, bc_epochs=5)
        m.current_epoch = 5
        m.enable_graph()
        m.log_every_n_steps = 50
        return m

    def timed(mod, next_batch):
        for _ in range(a.warmup):
            mod.training_step(next_batch(), 0)
        torch.cuda.synchronize()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
        evs[0].record()
        t0 = time.perf_counter()
        for i in range(a.steps):
            mod.training_step(next_batch(), 0)
            evs[i + 1].record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / a.steps * 1e3
        ts = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(a.steps))
        fin = bool(torch.isfinite(mod.engine.logs).all().item())
        mod._graphs = {}
        return {"ms_per_step": round(wall, 4), "p50_ms": round(ts[len(ts) // 2], 4), "p90_ms": round(ts[int(0.9 * len(ts))], 4),
                "max_ms": round(ts[-1], 4), "steps": a.steps, "losses_finite": fin}

    to_dev = lambda x: {k: to_dev(v) for k, v in x.items()} if isinstance(x, dict) else (x.to(dev) if torch.is_tensor(x) else x)  # noqa: E731
    out = {"config": f"C5: CQL_Offline B={B} n=32 84x84 {a.dtype}, hipGraph on", "device": torch.cuda.get_device_name(0),
           "dataset_frames": N}
    resident = to_dev(synth.make_transition_batch(7, B, {"rgb_static": (84, 84)}))
    out["a_resident_batch"] = timed(module(), lambda: resident)

    g = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 256, (N, 84, 84, 3), dtype=torch.uint8, generator=g)
    acts = np.random.RandomState(6).uniform(-1, 1, size=(N, 7)).astype(np.float32)
    acts[:, -1] = np.where(acts[:, -1] >= 0, 1.0, -1.0)
    nn = {s: np.random.RandomState(s).randint(0, N, size=32).tolist() for s in range(0, N, 2)}  # every other step has none
    ix = TransitionIndex([[i, i + 1999] for i in range(0, N, 2000)], n_frames=N, nn_steps_from_step=nn,
                         goal_strategy_prob={"geometric": 0.5, "similar_robot_obs": 0.5})  # the reference dataset's default
    rep = HbmTransitionReplay({"rgb_static": frames}, acts, ix, device=dev, batch_size=B)
    gen = torch.Generator(device=dev).manual_seed(7)
    spec = {"rgb_static": AugmentSpec(pad=4)}
    out["b_fed_from_transition_replay"] = timed(module(), lambda: rep.batch(ix.draw_device(B, dev, gen), fused=True))
    out["b_fed_with_augmentation"] = timed(module(), lambda: rep.batch(
        ix.draw_device(B, dev, gen), aug=draw_transition_batch_augmentation(spec, B, dev, gen), fused=True))
    rep.check()

    # (c) the sampler call alone, and the device draws in front of it
    d = ix.draw_device(B, dev, gen)
    for _ in range(20):
        rep.batch(d, fused=True)
    ev0, ev1, ev2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    ev0.record()
    for _ in range(1000):
        rep.batch(d, fused=True)
    ev1.record()
    for _ in range(1000):
        ix.draw_device(B, dev, gen)
    ev2.record()
    torch.cuda.synchronize()
    out["c_sampler_call_us"] = round(ev0.elapsed_time(ev1), 3)  # ms per 1000 launches = us per launch
    out["c_device_draws_us"] = round(ev1.elapsed_time(ev2), 3)
    # (d) the host sampler for the same B
    rng = np.random.default_rng(8)
    hd = [ix.draw(B, rng) for _ in range(200)]
    t0 = time.perf_counter()
    for x in hd:
        ix.sample(None, x)
    out["d_host_sample_us"] = round((time.perf_counter() - t0) / len(hd) * 1e6, 1)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
