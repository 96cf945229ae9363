"""Time the TACORL step fed by the play-window replays on one GPU (profiles/play_replay.md): the headline shape of bench.py
(B = 256, T = 16, 84x84, bf16 MFMA operands, the decoder frozen) and the batch of the reference's config/datamodule/tacorl.yaml
(B = 64, windows 8..16, goal strategies 0.9 / 0.1 with a neighbour table), the step captured as one hipGraph and replayed,
metrics read back every 50th step.

    python tools/time_play_replay.py [--steps 2000] [--warmup 100] [--only headline_b256] [--out FILE]

Per case ONE process, ONE module; the feeds alternate in rounds, so only the staging in front of the replayed graph differs:
  (a) one resident batch, the same tensors every step;
  (b) the host-sampled feed: prefetching(HbmReplay.batch(fused=True)) - NumPy sampling on a feeder thread, pinned staging ring,
      copy kernel on a private stream, an event wait per batch (data/replay.py);
  (c) HbmPlayReplay.batch(fused=True) on the trainer's thread, fresh device draws every step, no feeder (data/play_replay.py);
  (d) the same, dense (fused=False: the frames gathered into a uint8 batch first).
One HIP event per step; per feed the median, p10, p90, p99 and max of the per-step times and the wall clock.  Beside them, as
1 000 back-to-back calls each: `PlayIndex.draw_device` alone and one sampler launch (`batch(draws)`) alone.  Prints one JSON
line (and writes it to --out).  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"headline_b256": dict(B=256, min_ws=16, max_ws=16, strategy=None, nn=False),
         "yaml_b64": dict(B=64, min_ws=8, max_ws=16, strategy={"geometric": 0.9, "similar_robot_obs": 0.1}, nn=True)}
T, HW, N_FRAMES, EP_LEN = 16, 84, 40000, 2000  # bench.py --fed's dataset
_DATA = {}


def dataset(dev):
    if not _DATA:
        g = torch.Generator().manual_seed(5)
        _DATA["frames"] = torch.randint(0, 256, (N_FRAMES, HW, HW, 3), dtype=torch.uint8, generator=g).to(dev)
        _DATA["acts"] = np.random.RandomState(6).uniform(-1, 1, size=(N_FRAMES, 7)).astype(np.float32)
    return _DATA["frames"], _DATA["acts"]


def _stats(ts, wall_ms):
    ts = sorted(ts)
    q = lambda f: round(ts[min(len(ts) - 1, int(f * len(ts)))], 4)  # noqa: E731
    return {"median_ms": q(0.5), "p10_ms": q(0.1), "p90_ms": q(0.9), "p99_ms": q(0.99), "max_ms": round(ts[-1], 4),
            "wall_ms_per_step": round(wall_ms / len(ts), 4), "steps": len(ts)}


def timed_feeds(mod, feeds, steps, warmup, rounds=4):
    """feeds: {name: stream(n) -> an iterator of n batches}.  `rounds` rounds of steps / rounds timed steps per feed, `warmup`
    steps before a feed's first round and 10 after every switch; a feed's iterator is made anew for every round."""
    per = max(steps // rounds, 1)
    ts, wall = {k: [] for k in feeds}, {k: 0.0 for k in feeds}
    for r in range(rounds):
        for name, stream in feeds.items():
            warm = warmup if r == 0 else 10
            it = iter(stream(warm + per))
            for _ in range(warm):
                mod.training_step(next(it))
            torch.cuda.synchronize()
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(per + 1)]
            evs[0].record()
            t0 = time.perf_counter()
            for i in range(per):
                mod.training_step(next(it))
                evs[i + 1].record()
            torch.cuda.synchronize()
            wall[name] += (time.perf_counter() - t0) * 1e3
            ts[name] += [evs[i].elapsed_time(evs[i + 1]) for i in range(per)]
            for _ in it:  # (lets a feeder thread's generator finish and join)
                pass
    out = {k: _stats(ts[k], wall[k]) for k in feeds}
    out["graphs"], out["losses_finite"] = len(mod._graphs), bool(torch.isfinite(mod.engine.logs).all().item())
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


def case(cfg, dtype, dev, steps, warmup):
    import bench
    from tacorl_amd.data.neighbours import NeighbourTable
    from tacorl_amd.data.play_replay import HbmPlayReplay
    from tacorl_amd.data.replay import HbmReplay, PlayIndex, prefetching

    frames, acts = dataset(dev)
    B = cfg["B"]
    nn = None
    if cfg["nn"]:  # every fourth frame has 1..8 neighbours somewhere in the dataset
        rs = np.random.RandomState(8)
        nn = NeighbourTable.from_dict({k: rs.randint(0, N_FRAMES, size=rs.randint(1, 9)).tolist() for k in range(0, N_FRAMES, 4)},
                                      N_FRAMES)
    ix = PlayIndex([[i, i + EP_LEN - 1] for i in range(0, N_FRAMES, EP_LEN)], cfg["min_ws"], cfg["max_ws"], goal_sampling_prob=0.3,
                   goal_strategy_prob=cfg["strategy"], nn_steps_from_step=nn)
    old = HbmReplay({"rgb_static": frames}, acts, ix, dev)
    new = HbmPlayReplay({"rgb_static": frames}, acts, ix, device=dev, batch_size=B)
    rng = np.random.default_rng(7)
    resident = new.batch(fused=True)

    def host_fed(n):
        return prefetching(lambda: old.batch(rng.integers(len(ix), size=B), ix.draw(B, rng), fused=True), n)

    feeds = {"a_resident": lambda n: (resident for _ in range(n)),
             "b_host_prefetching": host_fed,
             "c_device_fused": lambda n: (new.batch(fused=True) for _ in range(n)),
             "d_device_dense": lambda n: (new.batch(fused=False) for _ in range(n))}
    mod = bench.build_module(torch.device(dev), dtype, T, 1)
    mod.enable_graph()
    mod.log_every_n_steps = 50
    out = timed_feeds(mod, feeds, steps, warmup)
    d = ix.draw_device(B, dev)
    out["sampler_launch_us"] = back_to_back(lambda: new.batch(d, fused=True))
    out["draw_device_us"] = back_to_back(lambda: ix.draw_device(B, dev))
    new.check()
    del mod
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--only", choices=sorted(CASES), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_play_replay: needs a GPU")
    from tacorl_amd import _lib

    dev = "cuda:0"
    _lib.call("tacorl_hip_init", 0)
    out = {"device": torch.cuda.get_device_name(0), "dtype": a.dtype, "T": T, "hw": HW, "dataset_frames": N_FRAMES, "hip_graph": True}
    for name, cfg in CASES.items():
        if a.only in (None, name):
            out[name] = case(cfg, a.dtype, dev, a.steps, a.warmup)
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
