"""The image-ingest stage of a tree, for a parent / head comparison (profiles/image_ingest_schedule.md):

  plan   every case of tests/test_image_ingest_gpu.py: its launch records (the PLAN literal of that test, --pprint), the
         sha256 of every image buffer the staging filled (module.frames[c], engine.X3[c]) and the step's logged scalars
  time   host time of TACORL._stage_frames alone, headline batch (fp32 NCHW, B = 256, window 16, 84 x 84, bf16 images) and
         the fused replay batch of the same shape: --calls calls after a warm-up, microseconds per call
  steps  --config c3 | c5 | playlmp_b32 | ril: 25 graph-mode training steps of that configuration (bf16), to be run under
         `rocprofv3 --kernel-trace --stats` for the kernel names and call counts
  stats  --csv A.csv B.csv: the kernels and calls of two rocprofv3 `*_kernel_stats.csv` files, and whether they are the same

--tree DIR imports tacorl_amd from DIR instead of this repository (another commit's Python over the same library); `tests`
and `bench` are always this repository's.  One JSON document on stdout (or --out FILE)."""
import argparse
import hashlib
import json
import os
import pprint
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Patch:
    def setattr(self, obj, name, value):
        setattr(obj, name, value)


def sha(t):
    import torch

    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


def plan(a):
    import torch

    from tests import test_image_ingest_gpu as I

    geo = I.geometry()
    rec = I.Recorder(_Patch())
    out = {"geometry": geo, "plan": {}, "hashes": {}, "scalars": {}, "seconds": {}}
    for name in sorted(I.cases(geo)):
        t0 = time.perf_counter()
        mod, records = I.run_case(rec, name, geo)
        torch.cuda.synchronize()
        out["seconds"][name] = round(time.perf_counter() - t0, 2)
        out["plan"][name] = records
        out["hashes"][name] = {k: sha(t) for k, t in sorted(I.buffers(mod).items())}
        out["scalars"][name] = {k: float(v).hex() for k, v in sorted(mod.logged.items())}
        mod._graphs = {}
        del mod
    if a.pprint:
        with open(a.pprint, "w") as f:
            f.write("PLAN = " + pprint.pformat(out["plan"], width=124, compact=True) + "\n")
    return out


def stage_time(a):
    import numpy as np
    import torch

    import bench
    from tacorl_amd.data.replay import HbmReplay, PlayIndex

    dev = torch.device("cuda:0")
    Bh, Th, H = 256, 16, 84
    mod = bench.build_module(dev, "bf16", Th, 1)
    g = torch.Generator().manual_seed(3)
    frames = torch.randint(0, 256, (4000, H, H, 3), dtype=torch.uint8, generator=g)
    acts = np.random.RandomState(4).uniform(-1, 1, size=(4000, 7)).astype(np.float32)
    ix = PlayIndex([[0, 3999]], Th, Th, goal_sampling_prob=0.3)
    rng = np.random.default_rng(1)
    hbm = HbmReplay({"rgb_static": frames}, acts, ix, device=dev)
    batches = {"headline_f32_nchw": bench.synth_batch(Bh, Th, H, H, dev, bench.DATA_SEED),
               "fused_replay": hbm.batch(rng.integers(len(ix), size=Bh), ix.draw(Bh, rng), fused=True)}
    out = {}
    for name, b in batches.items():
        for _ in range(20):
            mod._stage_frames(b, None)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            mod._stage_frames(b, None)
            ts.append(time.perf_counter() - t0)
            if len(ts) % 25 == 0:
                torch.cuda.synchronize()  # (outside the timed region: the launch queue never fills)
        torch.cuda.synchronize()
        ts = np.asarray(ts) * 1e6
        out[name] = {"calls": a.calls, "median_us": round(float(np.median(ts)), 2), "p10_us": round(float(np.percentile(ts, 10)), 2),
                     "p90_us": round(float(np.percentile(ts, 90)), 2)}
    return out


def steps(a):
    """C3: TACORL, decoder fine-tuned, B = 256, window 16; C5: CQL_Offline n = 32, B = 1024; PlayLMP B = 32, window 16;
    RelayImitationLearning B = 64 - all 84 x 84, bf16, as bench.time_other_configs / profiles/encoder_stage_schedule.md."""
    import torch

    import bench
    from tacorl_amd import synth
    from tests import ril_util as U

    dev, cams = torch.device("cuda:0"), {"rgb_static": (84, 84)}
    to_dev = lambda x: {k: to_dev(v) for k, v in x.items()} if isinstance(x, dict) else (x.to(dev) if torch.is_tensor(x) else x)  # noqa: E731
    args = ()
    if a.config == "c3":
        mod, batch = bench.build_module(dev, "bf16", 16, 1, finetune=True), bench.synth_batch(256, 16, 84, 84, dev, bench.DATA_SEED)
    elif a.config == "playlmp_b32":
        from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP
        from tests import cfg_util as C

        torch.manual_seed(bench.PARAM_SEED)
        cfg = C.playlmp_cfg(device=dev, compute_dtype="bf16", image_dtype="bf16")
        mod = PlayLMP(**{k: v for k, v in cfg.items() if k not in ("_target_", "_recursive_")})
        batch, args = bench.synth_batch(32, 16, 84, 84, dev, bench.DATA_SEED), (0,)
    elif a.config == "c5":
        from tacorl_amd.modules.cql.cql_offline_lightning import CQL_Offline
        from tests import cfg_util as C

        torch.manual_seed(bench.PARAM_SEED)
        cfg = C.cql_cfg(device=dev, compute_dtype="bf16", image_dtype="bf16", n_action_samples=32)
        mod = CQL_Offline(**{k: v for k, v in cfg.items() if k not in ("_target_", "_recursive_")})
        mod.current_epoch = 5
        batch, args = to_dev(synth.make_transition_batch(7, 1024, cams)), (0,)
    else:
        from tacorl_amd.modules.relay_imitation_learning.relay_imitation_learning import RelayImitationLearning

        torch.manual_seed(bench.PARAM_SEED)
        mod = RelayImitationLearning(device=dev, compute_dtype="bf16", image_dtype="bf16", **U.ril_cfg())
        batch, args = to_dev(U.make_ril_batch(7, 64, cams)), (0,)
    mod.enable_graph()
    mod.log_every_n_steps = 50
    for _ in range(25):
        mod.training_step(batch, *args)
    torch.cuda.synchronize()
    return {"config": a.config, "steps": 25}


def stats(a):
    import csv

    def read(path):
        with open(path) as f:
            return {r["Name"]: int(r["Calls"]) for r in csv.DictReader(f)}

    x, y = read(a.csv[0]), read(a.csv[1])
    pack = lambda d: {k: v for k, v in d.items() if "pack" in k.lower()}  # noqa: E731
    return {"first": {"kernels": len(x), "calls": sum(x.values())}, "second": {"kernels": len(y), "calls": sum(y.values())},
            "identical": x == y, "differ": {k: (x.get(k), y.get(k)) for k in sorted(set(x) | set(y)) if x.get(k) != y.get(k)},
            "pack_kernels": pack(x)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("what", choices=["plan", "time", "steps", "stats"])
    p.add_argument("--tree", default=ROOT)
    p.add_argument("--out")
    p.add_argument("--pprint", help="plan: also write the PLAN literal of the test to this file")
    p.add_argument("--calls", type=int, default=200)
    p.add_argument("--config", choices=["c3", "c5", "playlmp_b32", "ril"])
    p.add_argument("--csv", nargs=2)
    a = p.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import tacorl_amd  # noqa: F401  (the package of --tree: its submodules follow its __path__ ...)

    sys.path[0] = ROOT  # ... and everything else - tests, bench - is this repository's
    res = {"tree": os.path.abspath(a.tree), a.what: {"plan": plan, "time": stage_time, "steps": steps, "stats": stats}[a.what](a)}
    text = json.dumps(res, indent=1, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
