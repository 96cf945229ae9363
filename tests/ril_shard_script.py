"""Two ranks: a RelayImitationLearning training step on per-sample SHARDS (2 + 2 samples) must produce the gradients,
parameters and logged scalars of the single-rank step on the FULL batch (B = 4), hipGraph on (two collective-free graph
segments around the one gradient all-reduce).  Launched by tests/test_ril_gpu.py through torch.distributed.run with 2
processes, one GPU per rank (backend nccl = RCCL; TACORL_RIL_SHARD_BACKEND=gloo puts both ranks on cuda:0 for boxes with one
GPU).  Every loss is a batch mean, the loss kernel pre-scales its gradient by 1/world and the collective is a sum, so shard
and full agree to summation order - the bounds of tests/dist_shard_script.py."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tacorl_amd import dist as D  # noqa: E402
from tests import ril_util as U  # noqa: E402
from tests.golden_util import Golden  # noqa: E402
from tests.test_step_gpu import to_dev  # noqa: E402


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def build(g, world, dev):
    from tacorl_amd.modules.relay_imitation_learning.relay_imitation_learning import RelayImitationLearning

    mod = RelayImitationLearning(device=dev, world_size=world, **U.cfg_of_golden(g))
    mod.load_state_dict(g.params())
    return mod


def steps(mod, batch):
    mod.enable_graph()
    for _ in range(2):  # eager warm-up + capture, then a replay: both are training steps
        mod.training_step(to_dev(batch, mod.device), 0)
    torch.cuda.synchronize()
    return ({k: v.detach().clone() for k, v in mod.named_gradients().items()},
            {k: v.detach().clone() for k, v in mod.state_dict().items()}, dict(mod.logged))


def main():
    backend = os.environ.get("TACORL_RIL_SHARD_BACKEND", "nccl")
    dev = f"cuda:{int(os.environ.get('LOCAL_RANK', '0')) if backend == 'nccl' else 0}"
    torch.cuda.set_device(dev)
    dist.init_process_group(backend)
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    for name in U.GOLDENS:
        g = Golden(name)
        lr = g.cfg["lr"]
        batch = U.make_ril_batch(g.cfg["seed"] * 100, 4, g.cams)
        full = build(g, 1, dev)
        g_full, p_full, l_full = steps(full, batch)
        del full
        mod = build(g, 2, dev)
        g_sh, p_sh, l_sh = steps(mod, D.shard_batch(batch, rank, world))
        bad = []
        gmax = max(x.norm() for x in g_full.values())
        for k, v in g_full.items():
            if v.norm() > 0 and rel(g_sh[k], v) > 1e-5 and (g_sh[k] - v).norm() > 1e-6 * gmax:
                bad.append(f"grad {k}: rel {rel(g_sh[k], v):.3g}")
        for k, v in p_full.items():
            d = (p_sh[k] - v).abs()
            if rel(p_sh[k], v) > 1e-5 and float(d.max()) > 4.2 * lr:
                bad.append(f"param {k}: rel {rel(p_sh[k], v):.3g} max|d| {float(d.max()):.3g}")
            elif rel(p_sh[k], v) > 1e-3:
                bad.append(f"param {k}: rel {rel(p_sh[k], v):.3g}")
        assert set(l_full) == set(l_sh) and len(l_full) == 3, (sorted(l_full), sorted(l_sh))
        bad += [f"log {k}: shards {l_sh[k]!r} full {v!r}" for k, v in l_full.items() if abs(l_sh[k] - v) > 2e-5 * max(abs(v), 1e-2)]
        (gs, _, _), = mod._graphs.values()
        assert len(gs) == 2, "two graph segments around the all-reduce"
        assert not bad, f"{name} rank {rank}: shard != full\n" + "\n".join(bad[:20])
        del mod
        torch.cuda.empty_cache()
        if rank == 0:
            print(f"{name}: shard == full ok", flush=True)
        dist.barrier()
    if rank == 0:
        print("ALL OK", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
