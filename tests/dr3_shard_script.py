"""Two ranks, one GPU (gloo): a CQL_Offline training step WITH the DR3 term on per-sample halves of a batch, with sharded
noise, must give the gradients, parameters and logged scalars of the single-rank step on the full batch - the term's
per-rank mean, scaled by 1 / world, sums to the full-batch gradient in the step's second all-reduce, and its logged value
is averaged over the ranks like every other scalar (no collective of its own).

Launched by tests/test_dr3_dist_gpu.py through torch.distributed.run with 2 processes; tests/dist_shard_script.py is the
model and lends its helpers and its tolerances (gradients 1e-5 norm-wise, parameters after the two Adam steps 1e-5 relative
or a few lr in single elements, logged scalars 2e-5).  The golden cql_dr3 has B = 3, which does not halve: the full batch is
B = 4, the golden's step-0 batch followed by the first sample of its step-1 batch (and their noise), two samples per rank."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tacorl_amd import dist as D  # noqa: E402
from tests import cfg_util as C  # noqa: E402
from tests.dist_shard_script import PER_SAMPLE_MAJOR, cat_noise, cat_tree, one_step, rel  # noqa: E402
from tests.golden_util import Golden  # noqa: E402

B_FULL, N_SAMPLES, LR_MAX = 4, 4, 3e-4


def head(tree, n):
    """The first n samples of a batch tree (leading dimension)."""
    if isinstance(tree, dict):
        return {k: head(v, n) for k, v in tree.items()}
    return tree[:n].contiguous() if torch.is_tensor(tree) and tree.dim() > 0 else tree


def head_noise(noise, n, n_samples):
    out = {}
    for k, v in noise.items():
        if k in PER_SAMPLE_MAJOR:
            out[k] = v[:, :n].contiguous()
        elif k == "u_rand":
            out[k] = v.view(n_samples, v.shape[0] // n_samples, -1)[:, :n].reshape(n_samples * n, -1)
        else:
            out[k] = v[:n].contiguous()
    return out


def build(g, world):
    from tacorl_amd.lightning import instantiate

    return instantiate(C.cql_cfg(device="cuda:0", world_size=world, **g.cfg["overrides"]))


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    torch.cuda.set_device(0)
    g = Golden("cql_dr3")
    batch = head(cat_tree(g.batch(0), g.batch(1)), B_FULL)
    noise = head_noise(cat_noise(g.noise(0), g.noise(1), N_SAMPLES), B_FULL, N_SAMPLES)
    params0 = g.params()
    full = build(g, 1)
    assert full.engine.dr3 is not None
    full.load_state_dict(params0, strict=False)
    g_full, p_full, l_full = one_step("cql", full, g, batch, noise)
    del full
    mod = build(g, 2)
    mod.load_state_dict(params0, strict=False)
    sb, sn = D.shard_batch(batch, rank, world), D.shard_noise(noise, rank, world, N_SAMPLES)
    assert sb["actions"].shape[0] == B_FULL // 2
    g_sh, p_sh, l_sh = one_step("cql", mod, g, sb, sn)
    bad = []
    for k, v in g_full.items():
        if v.norm() > 0 and rel(g_sh[k], v) > 1e-5:
            if (g_sh[k] - v).norm() > 1e-6 * max(x.norm() for x in g_full.values()):
                bad.append(f"grad {k}: rel {rel(g_sh[k], v):.3g}")
    for k, v in p_full.items():
        d = (p_sh[k] - v).abs()
        if rel(p_sh[k], v) > 1e-5 and float(d.max()) > 4.2 * LR_MAX:
            bad.append(f"param {k}: rel {rel(p_sh[k], v):.3g} max|d| {float(d.max()):.3g}")
        elif rel(p_sh[k], v) > 1e-3:
            bad.append(f"param {k}: rel {rel(p_sh[k], v):.3g}")
    assert {"train/q1_dr3_loss", "train/q2_dr3_loss"} <= set(l_full) and set(l_full) <= set(l_sh), sorted(l_full)
    for k, v in l_full.items():
        if abs(l_sh[k] - v) > 2e-5 * max(abs(v), 1e-2):
            bad.append(f"log {k}: shards {l_sh[k]!r} full {v!r}")
    assert all(abs(l_full[f"train/{k}_dr3_loss"]) >= 1e-2 for k in ("q1", "q2")), l_full
    assert not bad, f"cql_dr3 rank {rank}: shard != full\n" + "\n".join(bad[:20])
    dist.barrier()
    if rank == 0:
        print("cql_dr3: shard == full ok (q1_dr3_loss %.6g)" % l_full["train/q1_dr3_loss"], flush=True)
        print("ALL OK", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
