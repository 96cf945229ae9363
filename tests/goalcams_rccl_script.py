"""CQL_Offline with goal cameras that differ from the observation cameras, RCCL on the step's path with ONE rank
(tests/rccl_one_rank_script.py has the symmetric modules): backend nccl, world_size 1, TACORL_FORCE_COLLECTIVES=1 - the
parameter broadcast, the alpha all-reduce and the gradient arena's (whose actor / q1 / q2 blocks have the asymmetric sizes)
between the hipGraph segments of three graph-mode steps must end where the collective-free single-graph steps end.
Launched by tests/test_goalcams_gpu.py; prints `ALL OK`."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import goalcams_util as U  # noqa: E402
from tests.dist_shard_script import rel  # noqa: E402
from tests.golden_util import Golden  # noqa: E402
from tests.rccl_one_rank_script import rccl_mapped, steps  # noqa: E402


def main():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29543")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    t = torch.ones(8, device="cuda")
    dist.all_reduce(t)  # communicator init
    torch.cuda.synchronize()
    libs = rccl_mapped()
    assert libs, "librccl is not mapped into the process after an nccl all-reduce"
    print("rccl:", libs, flush=True)
    g = Golden(U.NAME)
    obs_c, goal_c = g.cfg["obs_cams"], g.cfg["goal_cams"]
    os.environ["TACORL_FORCE_COLLECTIVES"] = "0"
    os.environ["TACORL_GRAPH_COLLECTIVES"] = "0"
    ref = U.build(obs_c, goal_c, world_size=1)
    ref.load_state_dict(g.params())
    g_ref, p_ref, l_ref, ng_ref = steps("cql", ref, g)
    assert ng_ref and all(n == 1 for n in ng_ref), ng_ref
    del ref
    os.environ["TACORL_FORCE_COLLECTIVES"] = "1"
    calls, orig = {"n": 0}, dist.all_reduce

    def counted(*a, **k):
        calls["n"] += 1
        return orig(*a, **k)

    dist.all_reduce = counted
    try:
        mod = U.build(obs_c, goal_c, world_size=1)
        mod.load_state_dict(g.params())
        g_c, p_c, l_c, ng_c = steps("cql", mod, g)
    finally:
        dist.all_reduce = orig
    assert ng_c and all(n >= 3 for n in ng_c), ng_c
    assert calls["n"] >= 6, calls
    bad = [f"grad {k}: rel {rel(g_c[k], v):.3g}" for k, v in g_ref.items() if v.norm() > 0 and rel(g_c[k], v) > 1e-6]
    bad += [f"param {k}: rel {rel(p_c[k], v):.3g}" for k, v in p_ref.items() if rel(p_c[k], v) > 1e-6]
    for a, b in zip(l_ref, l_c):
        bad += [f"log {k}: {b[k]!r} vs {v!r}" for k, v in a.items() if abs(b[k] - v) > 1e-6 * max(abs(v), 1e-3)]
    assert not bad, "collective step != collective-free step\n" + "\n".join(bad[:20])
    print(f"graphs/step {ng_c}, all_reduce calls {calls['n']}", flush=True)
    print("ALL OK", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
