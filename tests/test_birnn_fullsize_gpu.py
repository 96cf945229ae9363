"""The bidirectional-RNN plan recognition (`plan_recognition=tanh_net`) at the benchmarked sizes in bf16 - the ring-GEMM path:
PlayLMP at B = 32 (BASELINE configs[0], C1) with the early weight preparation and the in-launch plan sample, and TACORL at
B = 256 (configs[1], C2), both against the oracle with the bi-RNN posterior (tests/test_birnn_cpu.py) under bf16 operand
rounding, at the tolerances tests/test_fullsize_gpu.py holds the transformer path to; PlayLMP's captured graph against its
eager step."""
import copy

import pytest
import torch

from tests import cfg_util as C
from tests.test_birnn_cpu import TANH_NET, birnn_oracle  # noqa: F401  (fixture)
from tests.test_fullsize_gpu import _bf16_grad_check, _compare, _cpu, _logs, _noise, _to_dev

pytestmark = pytest.mark.gpu


def _strip(c):
    return {k: v for k, v in c.items() if k not in ("_target_", "_recursive_")}


def _playlmp(B_seed, compute="bf16"):
    from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP

    torch.manual_seed(B_seed)
    return PlayLMP(**_strip(C.playlmp_cfg(device="cuda:0", compute_dtype=compute, image_dtype=compute,
                                          plan_recognition=dict(TANH_NET))))


def test_playlmp_tanh_net_c1_bf16_vs_rounded_oracle(birnn_oracle):  # noqa: F811
    """C1 (B = 32, 84x84, window 16) in bf16: logged losses to 2e-3 (accuracies within 3 of 480 decisions) and every
    gradient norm-wise to 1e-2 or 3x its reproducibility floor."""
    from tacorl_amd import synth

    O = birnn_oracle
    mod = _playlmp(4)
    P = {k: v.detach().cpu().clone().contiguous() for k, v in mod.state_dict().items() if v.dtype == torch.float32}
    P = {k: v for k, v in P.items() if k in dict(mod.named_parameters())}
    O.require_grad_(P)
    opt = O.Adam([n for n in P], 1e-4)
    batch = synth.make_play_batch(4400, 32, 16, {"rgb_static": (84, 84)})
    mod.logged = {}
    mod.training_step(_to_dev(batch, mod.device), 0)
    torch.cuda.synchronize()
    assert mod.pr._ringed  # (the bf16 ring path ran)
    got = {k.split("/", 1)[1]: float(v) for k, v in mod.logged.items()}
    nz = {k: v.cpu().clone() for k, v in mod.noise.items()}
    g = torch.Generator().manual_seed(9)
    nz["rand"] = [torch.rand(32, 15, 6, 10, generator=g), torch.rand(32, 15, 6, generator=g),
                  torch.rand(32, 15, 6, 10, generator=g), torch.rand(32, 15, 6, generator=g)]
    nz["u_goal"] = torch.rand(32, 32, generator=g)
    with O.operand_rounding(torch.bfloat16):
        ologs, ograds = O.playlmp_step(P, opt, batch, nz, ["rgb_static"], step=False)
    bad = _compare(got, ologs, 2e-3, min_common=5, acc_atol=3.0 / (32 * 15))
    ev = lambda Pp: O.playlmp_step(Pp, opt, batch, nz, ["rgb_static"], step=False)[1]  # noqa: E731
    bad += _bf16_grad_check(mod, ev, ev, P, ograds)
    assert not bad, "\n".join(bad[:30])


def test_playlmp_tanh_net_graph_equals_eager():
    """bf16 PlayLMP steps with tanh_net, captured (first step: warm-up + capture, then replays) and eager, from the same
    parameters and noise: the same kernels on the same inputs, so logs, gradients and parameters agree bit for bit."""
    import bench

    batch = bench.synth_batch(32, 16, 84, 84, torch.device("cuda:0"), 1)
    res = []
    for graph in (True, False):
        m = _playlmp(0)
        if graph:
            m.enable_graph()
        torch.manual_seed(5)
        torch.cuda.manual_seed(5)
        for _ in range(3):
            m.training_step(batch, 0)
        torch.cuda.synchronize()
        res.append((dict(m.logged), {k: v.clone() for k, v in m.named_gradients().items()},
                    {k: v.clone() for k, v in m.state_dict().items()}))
    (la, ga, pa), (lb, gb, pb) = res
    assert la == lb and all(v == v for v in la.values()), (la, lb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k


def test_tacorl_tanh_net_c2_bf16_vs_rounded_oracle(birnn_oracle):  # noqa: F811
    """C2 (the headline shape: B = 256, window 16, frozen LMP) with tanh_net in bf16: losses and plans to 2e-3, every
    gradient norm-wise to 1e-2 or 3x its reproducibility floor."""
    from tacorl_amd import synth
    from tacorl_amd.modules.tacorl.tacorl import TACORL
    from tests.test_fullsize_gpu import _tacorl_oracle
    from tests.test_step_gpu import _snap

    cams = {"rgb_static": (84, 84)}
    lmp = _playlmp(3)
    mod = TACORL(play_lmp=lmp, finetune_action_decoder=False, critic=_strip(C.CRITIC), real_world=True, device="cuda:0",
                 compute_dtype="bf16", image_dtype="bf16", action_decoder_lr=3e-4, actor_lr=1e-4, critic_lr=3e-4,
                 discount=0.95, conservative_weight=1.0, reward_scale=10.0, n_action_samples=4, with_lagrange=True,
                 deterministic_backup=True, bc_epochs=5)
    mod.current_epoch = 5
    O, spec, P = _tacorl_oracle(mod, cams, 16, False)
    opts = O.make_opts(P, spec)
    batch = synth.make_play_batch(4302, 256, 16, cams)
    mod.logged = {}
    mod.training_step(_to_dev(batch, mod.device))
    got, nz = _logs(mod), _cpu(_noise(mod))
    assert mod.pr._ringed
    before, opts0 = _snap(P), copy.deepcopy(opts)
    with O.operand_rounding(torch.bfloat16):
        ologs, oplan, ograds = O.tacorl_step(P, opts, spec, batch, nz, 5)
    bad = _compare(got, ologs, 2e-3, plan=mod.plan, oplan=oplan)
    ev = lambda Pp: O.tacorl_step(Pp, copy.deepcopy(opts0), spec, batch, nz, 5)[2]  # noqa: E731
    bad += _bf16_grad_check(mod, ev, ev, before, ograds)
    assert not bad, "\n".join(bad[:30])
