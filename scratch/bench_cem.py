"""CEMOptimizer.get_action (one fused launch, csrc/cem_ops.hip) against the plain-torch restatement of the reference's
algorithm on the same GPU: the three in-scope shapes (CQL A=7 E=64, TACORL A=16 E=64, C4 A=32 E=128) at N = 256 and
4 iterations, f32 and bf16, R = 1 and R = 16 observation rows, embedding-level input on both sides.

Baseline = modules/cem.py cem_restatement with stock torch ops (F.linear + F.silu Q head in the same dtype) and the
reference's per-iteration .item(); the reference refines one observation at a time, so R rows are R calls.  It is the
reference's algorithm with the image duplication already removed - not tuned, and not the code under test.
HIP events around each call, --warmup calls first, median of --calls (>= 100) calls.
    python scratch/bench_cem.py [--calls 200] [--warmup 20]
    python scratch/bench_cem.py --one f32      # one warmed call of the TACORL shape, for rocprofv3 --kernel-trace --stats"""
import argparse
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tacorl_amd import _lib, engine  # noqa: E402
from tacorl_amd._lib import ACT_NONE, ACT_SILU, BF16, F32  # noqa: E402
from tacorl_amd.modules.cem import CEMOptimizer, cem_restatement  # noqa: E402
from tacorl_amd.modules.inference import CriticSurface  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--one", choices=("f32", "bf16"))
a = ap.parse_args()
_lib.call("tacorl_hip_init", 0)
dev = torch.device("cuda:0")
N, ITERS = 256, 4


def critics(A, E, compute):
    cams = ["rgb_static"] * 1 if E == 64 else ["rgb_gripper", "rgb_static"]
    owner = types.SimpleNamespace(dev=dev, compute=compute, img_dtype=torch.float32)
    qn = [(f"critic.Q.fc_layers.{i}.weight", f"critic.Q.fc_layers.{i}.bias") for i in range(3)] + [("critic.Q.out.weight", "critic.Q.out.bias")]
    out = []
    for seed in (1, 2):
        net = engine.NetBlock(cams, cams, [E + A, 256, 256, 256, 1], [ACT_SILU] * 3 + [ACT_NONE], qn, dev)
        gen = torch.Generator(device=dev).manual_seed(seed)
        for k, v in net.views.items():
            if k.startswith("critic."):
                v.copy_((torch.rand(v.shape, device=dev, generator=gen) * 2 - 1) / (v.shape[-1] ** 0.5 if v.dim() > 1 else 20.0))
        out.append(CriticSurface(owner, net, cams, cams, A))
    return out


def torch_q(surf, dtype):
    v = surf.net.views
    layers = [(v[f"critic.Q.fc_layers.{i}.weight"].to(dtype), v[f"critic.Q.fc_layers.{i}.bias"].to(dtype)) for i in range(3)]
    wo, bo = v["critic.Q.out.weight"].to(dtype), v["critic.Q.out.bias"].to(dtype)

    def q(emb, actions):
        x = torch.cat([emb.to(dtype).expand(actions.shape[0], -1), actions.to(dtype)], dim=-1)
        for w, b in layers:
            x = F.silu(F.linear(x, w, b))
        return F.linear(x, wo, bo).float()

    return q


def median_ms(fn):
    ts = []
    for i in range(a.warmup + a.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


if a.one:
    s1, s2 = critics(16, 64, BF16 if a.one == "bf16" else F32)
    cem = CEMOptimizer(s1, s2, batch_size=N, num_iterations=ITERS, action_dim=16)
    emb = torch.randn(1, 64, device=dev)
    for _ in range(3):
        cem.get_action(emb)
    torch.cuda.synchronize()
    sys.exit(0)

print(f"N = {N}, {ITERS} iterations, median of {a.calls} calls after {a.warmup}; times in ms per get_action over all R rows")
for shape, A, E in (("CQL", 7, 64), ("TACORL", 16, 64), ("C4", 32, 128)):
    for cname, compute, dtype in (("f32", F32, torch.float32), ("bf16", BF16, torch.bfloat16)):
        s1, s2 = critics(A, E, compute)
        q1, q2 = torch_q(s1, dtype), torch_q(s2, dtype)
        for twin in (False, True):
            cem = CEMOptimizer(s1, s2, batch_size=N, num_iterations=ITERS, action_dim=A, discrete_gripper=shape == "CQL", twin_min=twin)
            q_fn = (lambda e, x: torch.minimum(q1(e, x), q2(e, x))) if twin else q1
            for R in (1, 16):
                emb, mean0 = torch.randn(R, E, device=dev), 0.3 * torch.randn(R, A, device=dev)
                eps = torch.randn(R, ITERS, N, A, device=dev)
                fused = median_ms(lambda: cem.get_action(emb, initial_mean=mean0, noise={"eps": eps}))

                def base():
                    for r in range(R):
                        cem_restatement(q_fn, emb[r: r + 1], mean0[r], eps[r], n_elite=cem.n_elite, discrete_gripper=shape == "CQL",
                                        host_sync=True)

                torch_ms = median_ms(base)
                print(f"{shape:6s} A={A:2d} E={E:3d} {cname:4s} {'min(q1,q2)' if twin else 'q1        '} R={R:2d}: fused {fused:8.4f}  "
                      f"torch restatement {torch_ms:8.4f}  ratio {torch_ms / fused:6.2f}x", flush=True)
