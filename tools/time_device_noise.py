"""Time the eager prefix of the TACORL step - the staging in front of the captured graph: image pack, reward / done / actions,
the step's noise - at the benchmark's C2 shape (B = 256, T = 16, 84 x 84, bf16; bench.build_module / bench.synth_batch), with
torch's device generator (two launches) and with `device_noise_seed` (one tacorl_noise_fill launch), and the noise launches
alone.  HIP events around back-to-back calls, alternating rounds of the two forms in one process; medians over rounds.

    python tools/time_device_noise.py [--rounds 7] [--iters 200] [--out FILE]

On a tree without the feature (no TACORL.set_device_noise) only the torch form is timed.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(iters):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) * 1e3 / iters  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench

    dev = "cuda:0"
    mod = bench.build_module(dev, "bf16", 16, 1)
    batch = bench.synth_batch(a.batch, 16, 84, 84, dev, bench.DATA_SEED)
    mod.training_step(batch)  # sizes every buffer
    torch.cuda.synchronize()
    seeded = hasattr(mod, "set_device_noise")
    forms = {"torch": None, **({"device_noise": 11} if seeded else {})}
    res = {k: {"prefix_us": [], "noise_us": []} for k in forms}
    for _ in range(a.rounds):
        for k, seed in forms.items():
            if seeded:
                mod.set_device_noise(seed)
            res[k]["prefix_us"].append(timed(lambda: mod._stage_frames(batch, None, True, fold=getattr(mod, "fp32_ingest", True)), a.iters))
            res[k]["noise_us"].append(timed(lambda: mod.engine.set_noise(None), a.iters))
    out = {"shape": {"B": a.batch, "T": 16, "hw": 84, "dtype": "bf16"}, "rounds": a.rounds, "iters": a.iters,
           "noise_floats": int(mod.engine._noise_normal.numel() + mod.engine._noise_uniform.numel())}
    for k, r in res.items():
        out[k] = {m: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for m, v in r.items()}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
