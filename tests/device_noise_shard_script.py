"""Two ranks, one GPU (gloo), NO noise tape: each rank fills the noise of its own shard from the shared `device_noise_seed`
(sample0 = rank x B_local), and the step must produce the parameters of the single-rank step on the FULL batch with the same
seed - TACORL with a frozen action decoder and CQL_Offline, hipGraph on.  The mechanism, the full batch (two golden batches
concatenated) and the tolerances are those of tests/dist_shard_script.py's taped comparison: gradients 1e-5 norm-wise,
parameters 1e-5 relative or a few lr on single elements, logged scalars 2e-5.

Launched by tests/test_device_noise_dist_gpu.py through torch.distributed.run with 2 processes."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tacorl_amd import dist as D  # noqa: E402
from tests import device_noise_util as U  # noqa: E402
from tests.dist_shard_script import build, cat_tree, rel  # noqa: E402
from tests.golden_util import Golden  # noqa: E402
from tests.test_step_gpu import to_dev  # noqa: E402


def two_steps(mod, g, batch, sample0):
    """Two training steps without a tape (eager warm-up + capture, then a replay); the noise buffers are checked against the
    restatement for this rank's samples after each."""
    if "epoch" in g.cfg:
        mod.current_epoch = g.cfg["epoch"]
    mod.enable_graph()
    for step in range(2):
        mod.training_step(to_dev(batch, mod.device))
        torch.cuda.synchronize()
        U.check_buffers(mod, mod.engine.B, U.SEED, step, sample0)
    grads = {k: v.detach().clone() for k, v in mod.named_gradients().items()}
    params = {k: v.detach().clone() for k, v in mod.state_dict().items() if v.dtype.is_floating_point}
    return grads, params, dict(mod.logged)


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    torch.cuda.set_device(0)
    for kind, name, lr_max in (("tacorl", "tacorl_q", 3e-4), ("cql", "cql_q", 3e-4)):
        g = Golden(name)
        assert not g.cfg.get("finetune_ad")
        batch = cat_tree(g.batch(0), g.batch(1))
        params0 = g.params()
        full = build(kind, g, 1)
        full.load_state_dict(params0, strict=False)
        full.set_device_noise(U.SEED)
        g_full, p_full, l_full = two_steps(full, g, batch, 0)
        B_full = full.engine.B
        del full
        mod = build(kind, g, 2)
        mod.load_state_dict(params0, strict=False)
        mod.set_device_noise(U.SEED)
        g_sh, p_sh, l_sh = two_steps(mod, g, D.shard_batch(batch, rank, world), rank * (B_full // world))
        bad = []
        for k, v in g_full.items():
            if v.norm() > 0 and rel(g_sh[k], v) > 1e-5:
                # a gradient that is noise-level small against its block is exempt (summation order is all it is)
                if (g_sh[k] - v).norm() > 1e-6 * max(x.norm() for x in g_full.values()):
                    bad.append(f"grad {k}: rel {rel(g_sh[k], v):.3g}")
        for k, v in p_full.items():
            d = (p_sh[k] - v).abs()
            if rel(p_sh[k], v) > 1e-5 and float(d.max()) > 4.2 * lr_max:
                bad.append(f"param {k}: rel {rel(p_sh[k], v):.3g} max|d| {float(d.max()):.3g}")
            elif rel(p_sh[k], v) > 1e-3:
                bad.append(f"param {k}: rel {rel(p_sh[k], v):.3g}")
        assert l_full and set(l_full) <= set(l_sh), f"{name}: logged keys differ: {sorted(set(l_full) - set(l_sh))}"
        for k, v in l_full.items():
            if abs(l_sh[k] - v) > 2e-5 * max(abs(v), 1e-2):
                bad.append(f"log {k}: shards {l_sh[k]!r} full {v!r}")
        moved = sum(float((p_full[k] - params0[k].to(p_full[k].device)).abs().max()) > 0 for k in p_full if k in params0)
        assert moved > 0, f"{name}: the step did not move any parameter"
        assert not bad, f"{name} rank {rank}: shard != full\n" + "\n".join(bad[:20])
        del mod
        torch.cuda.empty_cache()
        if rank == 0:
            print(f"{name}: seeded shards == seeded full batch ok", flush=True)
        dist.barrier()
    if rank == 0:
        print("ALL OK", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
