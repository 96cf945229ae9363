"""Time the vector-observation (D4RL) training steps on one GPU: TACORL on AntMaze with the action decoder fine-tuned
(config/module/tacorl_d4rl.yaml) at B = 64 - the batch size of the reference's config/datamodule/tacorl_d4rl.yaml - and at
B = 256, and PlayLMP on AntMaze (config/module/play_lmp_d4rl.yaml) at B = 64; window 8, latent plan 16, bf16 MFMA operands,
the step captured as one hipGraph and replayed, device batches, metrics read back every 50th step.

    python tools/time_d4rl_step.py [--steps 2000] [--warmup 100] [--only tacorl_b64] [--out FILE]

Per case: warm-up, then one HIP event per step around the timed replays; the median, p10 and p90 of the per-step times and
the wall clock over all of them.  Prints one JSON line (and writes it to --out).  `--only CASE` runs one case - the form to put
behind `rocprofv3 --kernel-trace --stats --` for the per-kernel shares (a run of its own: tracing serialises the graph's
branches, so its step time is not the untraced one).  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"tacorl_b64": ("tacorl", 64), "tacorl_b256": ("tacorl", 256), "playlmp_b64": ("playlmp", 64)}
T, LATENT = 8, 16


def build(kind, dtype, dev):
    from tests import d4rl_cfg as K

    torch.manual_seed(0)
    lmp = K.build(K.playlmp_d4rl_cfg(latent=LATENT, T=T, device=dev, compute_dtype=dtype))
    mod = lmp if kind == "playlmp" else K.build(K.tacorl_d4rl_cfg(play_lmp=lmp, finetune_action_decoder=True, device=dev,
                                                                  compute_dtype=dtype))
    mod.enable_graph()
    mod.log_every_n_steps = 50
    return mod


def timed(mod, batch, steps, warmup):
    for _ in range(warmup):
        mod.training_step(batch, 0)
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    evs[0].record()
    t0 = time.perf_counter()
    for i in range(steps):
        mod.training_step(batch, 0)
        evs[i + 1].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps * 1e3
    ts = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(steps))
    logs = mod.engine.logs if hasattr(mod, "engine") else mod.logs
    return {"median_ms": round(ts[len(ts) // 2], 4), "p10_ms": round(ts[len(ts) // 10], 4), "p90_ms": round(ts[int(0.9 * len(ts))], 4),
            "wall_ms_per_step": round(wall, 4), "steps": steps, "graphs": len(mod._graphs),
            "losses_finite": bool(torch.isfinite(logs).all().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--only", choices=sorted(CASES), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_d4rl_step: needs a GPU")
    from tacorl_amd import _lib, synth

    dev = "cuda:0"
    _lib.call("tacorl_hip_init", 0)
    out = {"device": torch.cuda.get_device_name(0), "dtype": a.dtype, "window": T, "latent_plan_dim": LATENT, "hip_graph": True}
    for name, (kind, B) in CASES.items():
        if a.only not in (None, name):
            continue
        batch = {k: v.to(dev) for k, v in synth.make_d4rl_window_batch(7, B, T).items()}
        mod = build(kind, a.dtype, dev)
        out[name] = timed(mod, batch, a.steps, a.warmup)
        del mod
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
