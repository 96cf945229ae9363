"""Time RelayImitationLearning at the configuration of profiles/ril_step.md (B = 64, one 84x84 camera, 4 x 1024 policies, Tanh
goal encoder, bf16, hipGraph on, metrics read back every 50 steps) fed four ways, on one GPU:

  (a) the step on a resident dense batch (the same fp32 NCHW tensors every step);
  (b) the step fed by HbmRelayReplay.batch(fused=True) with fresh device draws per step, without and with the train-time
      augmentation (four draws per camera and item);
  (c) the sampler alone: HbmRelayReplay.batch() = one tacorl_sample_relay launch, device events around back-to-back calls
      (an upper bound on the kernel: the calls are paced by the host), and the device draws;
  (d) the host sampler, RelayIndex.sample, for the same B (host clock).

    python tools/time_ril_replay.py [--steps 400] [--frames 40000] [--out FILE]

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
P = "tacorl.networks."


def ril_kwargs():
    """config/module/relay_imitation_learning.yaml, one camera."""
    enc = {"_target_": P + "visual_encoders.encoder.LMPVisionEncoder", "latent_dim": 32, "hidden_dim": 256, "normalize_output": False}

    def actor(dg, action_dim):
        c = {"_target_": P + "actor_critic.actor.Actor", "_recursive_": False, "action_dim": action_dim,
             "policy": {"_target_": P + "actor_critic.actor.MLPPolicy", "num_layers": 4, "hidden_dim": 1024}}
        return dict(c, discrete_gripper=True) if dg else c

    return dict(env={}, goal_encoder={"_target_": P + "visual_encoders.goal_encoder.VisualGoalEncoder", "in_features": None,
                                      "out_features": 32, "hidden_size": 256, "activation_function": "ReLU",
                                      "last_layer_activation": "Tanh"},
                perceptual_encoder={"_target_": P + "representation.representation_network.LateFusion", "_recursive_": False,
                                    "networks": {"rgb_static": enc}},
                high_level_policy=actor(False, 32), low_level_policy=actor(True, 7), high_level_policy_modalities=["rgb_static"],
                low_level_policy_modalities=["rgb_static"], lr=1e-4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=40000)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ril_replay: needs a GPU")
    from tacorl_amd import _lib
    from tacorl_amd.data.augment import AugmentSpec, draw_ril_batch_augmentation
    from tacorl_amd.data.relay_replay import SLOTS, HbmRelayReplay, RelayIndex
    from tacorl_amd.modules.relay_imitation_learning.relay_imitation_learning import RelayImitationLearning

    dev, B, N = "cuda:0", a.batch, a.frames
    _lib.call("tacorl_hip_init", 0)

    def module():
        torch.manual_seed(0)
        m = RelayImitationLearning(device=dev, compute_dtype=a.dtype, image_dtype=a.dtype, **ril_kwargs())
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

    out = {"config": f"RIL B={B} 84x84 4x1024 {a.dtype}, hipGraph on", "device": torch.cuda.get_device_name(0), "dataset_frames": N}
    g = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 256, (N, 84, 84, 3), dtype=torch.uint8, generator=g)
    acts = np.random.RandomState(6).uniform(-1, 1, size=(N, 7)).astype(np.float32)
    acts[:, -1] = np.where(acts[:, -1] >= 0, 1.0, -1.0)
    ix = RelayIndex([[i, i + 1999] for i in range(0, N, 2000)], n_frames=N)  # the yaml's windows: 30 / 260
    rep = HbmRelayReplay({"rgb_static": frames}, acts, ix, device=dev, batch_size=B)
    gen = torch.Generator(device=dev).manual_seed(7)

    # (a) one batch of the dataset's own frames, host-transformed to the reference's fp32 NCHW schema, resident
    first = rep.batch(ix.draw_device(B, dev, gen), fused=False)
    resident = {s: {"rgb_static": ((first[s]["rgb_static"].permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5).contiguous()} for s in SLOTS}
    resident["low_level_action"] = first["low_level_action"].clone()
    out["a_resident_batch"] = timed(module(), lambda: resident)

    spec = {"rgb_static": AugmentSpec(pad=4)}
    out["b_fed_from_relay_replay"] = timed(module(), lambda: rep.batch(ix.draw_device(B, dev, gen), fused=True))
    out["b_fed_with_augmentation"] = timed(module(), lambda: rep.batch(
        ix.draw_device(B, dev, gen), aug=draw_ril_batch_augmentation(spec, B, dev, gen), fused=True))
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
