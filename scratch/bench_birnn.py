"""PlayLMP.training_step and TACORL.training_step (frozen LMP, Q phase: the C2 shape at B = 256) with
plan_recognition=tanh_net (bidirectional ReLU-RNN) vs the default transformer, same process, bf16, synthetic inputs: median
step time over --steps timed steps after --warmup.  python scratch/bench_birnn.py [B ...] [--tacorl B] [--graph]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from tacorl_amd import _lib, synth  # noqa: E402
from tests import cfg_util as C  # noqa: E402

# config/networks/plan_recognition/tanh_net.yaml, ${latent_plan_dim} = 16
TANH_NET = {"_target_": "tacorl.networks.plan_encoders.plan_recognition_tanh_net.PlanRecognitionTanhNetwork",
            "state_dim": None, "latent_plan_dim": 16, "birnn_dropout_p": 0.0, "min_std": 0.0001}

ap = argparse.ArgumentParser()
ap.add_argument("batch", type=int, nargs="*", default=[32])
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--graph", action="store_true")
ap.add_argument("--tacorl", type=int, nargs="*", default=[256])
a = ap.parse_args()
_lib.call("tacorl_hip_init", 0)
from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP  # noqa: E402

strip = lambda c: {k: v for k, v in c.items() if k not in ("_target_", "_recursive_")}  # noqa: E731
from tacorl_amd.modules.tacorl.tacorl import TACORL  # noqa: E402


def timed(what, mod, step):
    if a.graph:
        mod.enable_graph()
    ts = []
    for i in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            ts.append(e0.elapsed_time(e1))
    print(f"{what} {'graph' if a.graph else 'eager'}: median {statistics.median(ts):.3f} ms/step over {len(ts)} steps", flush=True)


PRS = (("transformer", C.plan_recognition(16, 16)), ("tanh_net", dict(TANH_NET)))
for B in a.batch:
    batch = synth.make_play_batch(1, B, 16, {"rgb_static": (84, 84)})
    batch = {k: ({c: t.cuda() for c, t in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in batch.items()}
    for name, pr in PRS:
        mod = PlayLMP(**strip(C.playlmp_cfg(device="cuda:0", plan_recognition=pr)), compute_dtype="bf16", image_dtype="bf16")
        timed(f"PlayLMP B={B} {name:11s}", mod, lambda: mod.training_step(batch, 0))
        del mod
        torch.cuda.empty_cache()
for B in a.tacorl:
    batch = synth.make_play_batch(2, B, 16, {"rgb_static": (84, 84)})
    batch = {k: ({c: t.cuda() for c, t in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in batch.items()}
    for name, pr in PRS:
        lmp = PlayLMP(**strip(C.playlmp_cfg(device="cuda:0", plan_recognition=pr)), compute_dtype="bf16", image_dtype="bf16")
        mod = TACORL(play_lmp=lmp, **strip(C.tacorl_cfg(device="cuda:0", finetune_action_decoder=False)), compute_dtype="bf16",
                     image_dtype="bf16")
        mod.current_epoch = 5
        timed(f"TACORL  B={B} {name:11s}", mod, lambda: mod.training_step(batch))
        del mod, lmp
        torch.cuda.empty_cache()
