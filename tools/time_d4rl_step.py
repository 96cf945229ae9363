"""Time the vector-observation (D4RL) training steps on one GPU: TACORL on AntMaze with the action decoder fine-tuned
(config/module/tacorl_d4rl.yaml) at B = 64 - the batch size of the reference's config/datamodule/tacorl_d4rl.yaml - and at
B = 256, and PlayLMP on AntMaze (config/module/play_lmp_d4rl.yaml) at B = 64; window 8, latent plan 16, bf16 MFMA operands,
the step captured as one hipGraph and replayed, device batches, metrics read back every 50th step.

    python tools/time_d4rl_step.py [--steps 2000] [--warmup 100] [--only tacorl_b64] [--out FILE] [--fed]

Per case: warm-up, then one HIP event per step around the timed replays; the median, p10 and p90 of the per-step times and
the wall clock over all of them.  Prints one JSON line (and writes it to --out).  `--only CASE` runs one case - the form to put
behind `rocprofv3 --kernel-trace --stats --` for the per-kernel shares (a run of its own: tracing serialises the graph's
branches, so its step time is not the untraced one).  Needs a GPU: there is no fallback.

`--fed` (profiles/d4rl_replay.md): the same cases fed from a resident window replay (data/d4rl_replay.py HbmD4RLReplay) over a
synthetic dataset of 1 000 000 frames in episodes of 1 000.  One module and one captured graph per case; four feeds alternate
in rounds: (a) one resident batch - the plain measurement above, re-made in the same call -, (b) the dense replay batch, (c) the
fused batch, fresh device draws every step, (d) the host numpy sampler with CPU tensors copied by the step.  Beside them, as
1 000 back-to-back calls each: `batch()` alone and `draw_device` alone."""
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


_FED = {}


def fed_replay(kind, B, dev, n=1_000_000, ep=1000):
    """--fed: a synthetic dataset of n frames in episodes of `ep` (AntMaze's size and episode length), resident; TACORL's index
    samples goals (p = 0.3), PlayLMP's does not.  Window min = max = T, as the experiments set it."""
    import numpy as np

    from tacorl_amd.data.d4rl_replay import D4RLWindowIndex, HbmD4RLReplay

    if not _FED:
        rng = np.random.default_rng(0)
        _FED["obs"] = rng.random((n, 29), dtype=np.float32) * 16.0
        _FED["act"] = rng.random((n, 8), dtype=np.float32) * 2.0 - 1.0
        _FED["timeouts"] = np.zeros(n, dtype=bool)
        _FED["timeouts"][ep - 1::ep] = True
        _FED["dev"] = (torch.from_numpy(_FED["obs"]).to(dev), torch.from_numpy(_FED["act"]).to(dev))
    ix = D4RLWindowIndex(_FED["timeouts"], np.zeros(n, dtype=bool), min_window_size=T, max_window_size=T,
                         include_goal=kind == "tacorl", goal_sampling_prob=0.3)
    return HbmD4RLReplay(*_FED["dev"], ix, device=dev, batch_size=B)


def _stats(ts, wall_ms, n):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 4), "p10_ms": round(ts[len(ts) // 10], 4), "p90_ms": round(ts[int(0.9 * len(ts))], 4),
            "wall_ms_per_step": round(wall_ms / n, 4), "steps": n}


def timed_fed(mod, feeds, steps, warmup, rounds=4):
    """ONE module, one captured graph; the feeds alternate in `rounds` rounds of steps / rounds timed steps each (the staging in
    front of the replay is all that differs), `warmup` steps before a feed's first round and 10 after every switch."""
    per = max(steps // rounds, 1)
    ts, wall = {k: [] for k in feeds}, {k: 0.0 for k in feeds}
    for r in range(rounds):
        for name, nxt in feeds.items():
            for _ in range(warmup if r == 0 else 10):
                mod.training_step(nxt(), 0)
            torch.cuda.synchronize()
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(per + 1)]
            evs[0].record()
            t0 = time.perf_counter()
            for i in range(per):
                mod.training_step(nxt(), 0)
                evs[i + 1].record()
            torch.cuda.synchronize()
            wall[name] += (time.perf_counter() - t0) * 1e3
            ts[name] += [evs[i].elapsed_time(evs[i + 1]) for i in range(per)]
    logs = mod.engine.logs if hasattr(mod, "engine") else mod.logs
    out = {k: _stats(ts[k], wall[k], per * rounds) for k in feeds}
    out["graphs"], out["losses_finite"] = len(mod._graphs), bool(torch.isfinite(logs).all().item())
    return out


def back_to_back(fn, calls=1000):
    """us per call: device events around `calls` back-to-back calls (an upper bound: paced by the host's enqueue)."""
    for _ in range(50):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / calls * 1e3, 2)


def fed_case(kind, B, dtype, dev, steps, warmup):
    import numpy as np

    from tacorl_amd import synth

    rp = fed_replay(kind, B, dev)
    ix, rng = rp.index, np.random.default_rng(1)
    resident = {k: v.to(dev) for k, v in synth.make_d4rl_window_batch(7, B, T).items()}

    def host():  # what a Python feeder gives at best: the numpy sampler on the trainer's thread, CPU tensors copied by the step
        s = ix.sample(None, ix.draw(B, rng), _FED["obs"], _FED["act"])
        b = {"observations": torch.from_numpy(s["observations"]), "actions": torch.from_numpy(s["actions"])}
        if ix.include_goal:
            b.update(goal=torch.from_numpy(s["goal"]), goal_reached=torch.from_numpy(s["goal_reached"]))
        return b

    feeds = {"a_resident": lambda: resident, "b_dense": lambda: rp.batch(fused=False), "c_fused": lambda: rp.batch(fused=True),
             "d_host_numpy": host}
    mod = build(kind, dtype, dev)
    out = timed_fed(mod, feeds, steps, warmup)
    d = ix.draw_device(B, dev)
    out["batch_dense_us"] = back_to_back(lambda: rp.batch(d, fused=False))
    out["draw_device_us"] = back_to_back(lambda: ix.draw_device(B, dev))
    rp.check()
    del mod
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--only", choices=sorted(CASES), default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fed", action="store_true", help="feed the steps from a resident D4RL window replay (profiles/d4rl_replay.md)")
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
        if a.fed:
            out[name] = fed_case(kind, B, a.dtype, dev, a.steps, a.warmup)
        else:
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
