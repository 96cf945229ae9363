"""Two ranks, one GPU (gloo): a D4RL training step on per-sample SHARDS (2 + 2 samples) with sharded noise must produce the
gradients, parameters and logged scalars of the single-rank step on the FULL batch (B = 4) - TACORL on vector observations
with a frozen and with a fine-tuned action decoder (whose gradient block rides in the engine's arena: one scalar all-reduce plus
one arena all-reduce per step) and PlayLMP on vector observations - with the step captured as graph segments around the eager
all-reduces.  Launched by tests/test_d4rl_modules_gpu.py through torch.distributed.run with 2 processes; bounds and reasoning:
tests/dist_shard_script.py."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tacorl_amd import dist as D  # noqa: E402
from tests import d4rl_cfg as K  # noqa: E402
from tests.dist_shard_script import rel  # noqa: E402
from tests.test_step_gpu import to_dev  # noqa: E402

B, N_S = 4, 4


def build(kind, g, world):
    lmp = K.build(K.playlmp_d4rl_cfg(latent=g.cfg["latent"], T=g.cfg["T"], device="cuda:0", dropout_p=0.0, world_size=world))
    if kind == "playlmp":
        return lmp
    return K.build(K.tacorl_d4rl_cfg(play_lmp=lmp, finetune_action_decoder=g.cfg["finetune_ad"], device="cuda:0",
                                     world_size=world))


def make_noise(kind, seed, A=16):
    gen = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    if kind == "playlmp":
        return dict(eps_plan=n(B, A), u_plan=torch.rand(B, A, generator=gen))
    return dict(eps_pr=n(B, A), eps_pi=n(B, A), eps_next=n(B, A), u_rand=torch.rand(N_S * B, A, generator=gen),
                eps_cur=n(N_S, B, A), eps_nxt=n(N_S, B, A))


def one_step(mod, batch, noise):
    mod.enable_graph()
    for _ in range(2):  # first call: eager warm-up + capture, second: graph replay - both are training steps
        mod.training_step(to_dev(batch, mod.device), noise=to_dev(noise, mod.device))
    torch.cuda.synchronize()
    grads = {k: v.detach().clone() for k, v in mod.named_gradients().items()}
    params = {k: v.detach().clone() for k, v in mod.state_dict().items() if v.dtype.is_floating_point}
    return grads, params, dict(mod.logged)


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    torch.cuda.set_device(0)
    for kind, name, lr_max in (("tacorl", "tacorl_d4rl_q", 3e-4), ("tacorl", "tacorl_d4rl_ad", 3e-4), ("playlmp", "playlmp_d4rl", 1e-4)):
        g = K.D4rlGolden(name)
        batch, noise, params0 = g.batch(0, B=B), make_noise(kind, g.cfg["seed"]), g.params()
        assert batch["goal_reached"][:2].any() and not batch["goal_reached"][:2].all()
        full = build(kind, g, 1)
        full.load_state_dict(params0, strict=False)
        g_full, p_full, l_full = one_step(full, batch, noise)
        del full
        mod = build(kind, g, 2)
        mod.load_state_dict(params0, strict=False)
        g_sh, p_sh, l_sh = one_step(mod, D.shard_batch(batch, rank, world), D.shard_noise(noise, rank, world, N_S))
        bad = []
        for k, v in g_full.items():
            if v.norm() > 0 and rel(g_sh[k], v) > 1e-5:
                if (g_sh[k] - v).norm() > 1e-6 * max(x.norm() for x in g_full.values()):
                    bad.append(f"grad {k}: rel {rel(g_sh[k], v):.3g}")
        for k, v in p_full.items():
            d = (p_sh[k] - v).abs()
            if rel(p_sh[k], v) > 1e-5 and float(d.max()) > 4.2 * lr_max:
                bad.append(f"param {k}: rel {rel(p_sh[k], v):.3g} max|d| {float(d.max()):.3g}")
            elif rel(p_sh[k], v) > 1e-3:
                bad.append(f"param {k}: rel {rel(p_sh[k], v):.3g}")
        assert l_full and set(l_full) <= set(l_sh), f"{name}: logged keys differ: {sorted(set(l_full) - set(l_sh))}"
        bad += [f"log {k}: shards {l_sh[k]!r} full {v!r}" for k, v in l_full.items() if abs(l_sh[k] - v) > 2e-5 * max(abs(v), 1e-2)]
        moved = sum(float((p_full[k] - params0[k].to(p_full[k].device)).abs().max()) > 0 for k in p_full if k in params0)
        assert moved > 0, f"{name}: the step did not move any parameter"
        assert not bad, f"{name} rank {rank}: shard != full\n" + "\n".join(bad[:20])
        if kind == "tacorl":
            gs, _side, _ = next(iter(mod._graphs.values()))
            assert len(gs) == 3, "two ranks: three graph segments around the two all-reduces"
            if g.cfg["finetune_ad"]:
                assert any(k.startswith("action_decoder.") for k in g_full), "fine-tuned decoder gradients missing"
                a = mod.engine.grad_arena
                assert a.data_ptr() <= mod.ad.blk.grad.data_ptr() < a.data_ptr() + 4 * a.numel(), \
                    "the decoder's gradient block is not part of the arena (second collective)"
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
