"""RelayImitationLearning on the GPU against the goldens recorded from the unmodified reference module
(tools/gen_ril_golden.py): f32 parity over two free-running steps, bf16 mode, graph replay against eager, validation,
the summed obs-embedding gradient, uint8 frames, two-rank shards and a Trainer.fit smoke."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import ril_util as U
from tests.golden_util import Golden, check_stats
from tests.proc_util import free_port, run_group
from tests.test_step_gpu import L_as_list, check_logs, relerr, to_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-4  # the project's parity bar (f32 MFMA mode)


def build(g, **kw):
    from tacorl_amd.modules.relay_imitation_learning.relay_imitation_learning import RelayImitationLearning

    mod = RelayImitationLearning(device="cuda:0", **U.cfg_of_golden(g, **kw))
    mod.load_state_dict(g.params())
    return mod


def _step(mod, batch, train=True):
    mod.logged = {}
    (mod.training_step if train else mod.validation_step)(to_dev(batch, mod.device), 0)
    torch.cuda.synchronize()
    return {k.split("/", 1)[1]: v for k, v in mod.logged.items()}


@pytest.mark.parametrize("name", U.GOLDENS)
def test_ril_step_f32_parity(name):
    """Two optimiser steps, nothing re-synchronised in between: every logged scalar, every gradient fingerprint and every
    post-step parameter fingerprint of the reference within 1e-4 relative."""
    g = Golden(name)
    mod = build(g)
    assert sorted(mod.state_dict()) == sorted(g.names)
    for step in range(g.cfg["steps"]):
        got = _step(mod, U.golden_batch(g, step))
        exp = g.logged(step)
        assert set(exp) == set(got) == {"low_level_loss", "high_level_loss", "total_loss"}
        print(f"step {step}: " + ", ".join(f"{k} {got[k]:.8g} (ref {exp[k]:.8g})" for k in sorted(exp)))
        bad = check_logs(got, exp, RTOL)
        bad += check_stats(mod.named_gradients(), g.stats(step, "grad"), rtol=RTOL, what="grad ")
        bad += check_stats(mod.state_dict(), g.stats(step, "param"), rtol=RTOL, what="param ")
        assert len(g.stats(step, "grad")) == len(g.names) == len(g.stats(step, "param"))
        assert not bad, f"step {step}:\n" + "\n".join(bad[:25])
    assert int(mod.engine.blk.step) == g.cfg["steps"]


@pytest.mark.parametrize("name", U.GOLDENS)
def test_ril_step_bf16_mode(name):
    """bf16 MFMA operands (fused encoder, fused goal-encoder MLP, per-layer bf16 policies): finite, and the logged losses of
    the first step within 3e-2 of the fp32 reference - what tests/test_step_gpu.py allows the bf16 step against f32."""
    g = Golden(name)
    mod = build(g, compute_dtype="bf16", image_dtype="bf16")
    got = _step(mod, U.golden_batch(g, 0))
    print(", ".join(f"{k} {got[k]:.8g} (ref {v:.8g})" for k, v in sorted(g.logged(0).items())))
    bad = check_logs(got, g.logged(0), rtol=3e-2)
    assert not bad, "\n".join(bad)
    got = _step(mod, U.golden_batch(g, 1))
    assert all(np.isfinite(v) for v in got.values()), got
    assert all(torch.isfinite(v).all() for v in mod.state_dict().values())
    assert all(torch.isfinite(v).all() and v.abs().max() > 0 for v in mod.named_gradients().values())
    assert mod.engine.mlp_paths()["goal_encoder"] == ("fused", "fused")


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_graph_replay_equals_eager(compute):
    """Three eager steps against three steps in graph mode (warm-up + capture, then two replays): the same kernels on the
    same inputs, so logged scalars and parameters agree (the criterion of test_hipgraph_survives_batch_size_changes)."""
    g = Golden("ril_twocam")
    mods = [build(g, compute_dtype=compute, image_dtype=compute) for _ in range(2)]
    mods[0].enable_graph()
    for i in range(3):
        outs = [_step(m, U.golden_batch(g, i % 2)) for m in mods]
        bad = [f"{k}: graph {outs[0][k]:.9g} eager {outs[1][k]:.9g}" for k in outs[1]
               if abs(outs[0][k] - outs[1][k]) > 1e-6 * max(abs(outs[1][k]), 1e-3)]
        assert outs[0].keys() == outs[1].keys() and not bad, f"step {i}:\n" + "\n".join(bad)
    sd0, sd1 = mods[0].state_dict(), mods[1].state_dict()
    worst = max(relerr(sd0[k], sd1[k]) for k in sd0 if sd1[k].norm() > 0)
    assert worst < 1e-6, worst
    (gs, g_side, _), = mods[0]._graphs.values()
    assert len(gs) == 1 and g_side is None and int(mods[0].engine.blk.step) == 3
    # validation beside training: its own capture, the training graph survives
    v = [_step(m, U.golden_batch(g, 0), train=False) for m in mods]
    assert len(mods[0]._graphs) == 2 and all(abs(v[0][k] - v[1][k]) <= 1e-6 * max(abs(v[1][k]), 1e-3) for k in v[1])


def test_graph_split_at_the_gradient_all_reduce():
    """The form several ranks replay: two collective-free graph segments around the one gradient all-reduce."""
    g = Golden("ril")
    mods = [build(g) for _ in range(2)]
    mods[0]._force_graph_split = True
    mods[0].enable_graph()
    for i in range(2):
        outs = [_step(m, U.golden_batch(g, i)) for m in mods]
        assert all(abs(outs[0][k] - outs[1][k]) <= 1e-6 * max(abs(outs[1][k]), 1e-3) for k in outs[1]), outs
    (gs, _, _), = mods[0]._graphs.values()
    assert len(gs) == 2
    sd0, sd1 = mods[0].state_dict(), mods[1].state_dict()
    assert max(relerr(sd0[k], sd1[k]) for k in sd0 if sd1[k].norm() > 0) < 1e-6


def test_validation_step_moves_nothing():
    g = Golden("ril")
    mod = build(g)
    mod.eval()
    before = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    opt_before = [o.state_dict() for o in L_as_list(mod.configure_optimizers())]
    mod.logged = {}
    out = mod.validation_step(to_dev(U.golden_batch(g, 0), mod.device), 0)
    torch.cuda.synchronize()
    assert sorted(mod.logged) == ["validation/high_level_loss", "validation/low_level_loss", "validation/total_loss"]
    assert out == mod.logged["validation/total_loss"]
    # the same parameters and batch as the golden's first training step: the losses are that step's
    bad = check_logs({k.split("/", 1)[1]: v for k, v in mod.logged.items()}, g.logged(0), RTOL)
    after = mod.state_dict()
    bad += [f"{k} moved" for k, v in before.items() if not torch.equal(v, after[k])]
    for o0, o in zip(opt_before, L_as_list(mod.configure_optimizers())):
        s1 = o.state_dict()["state"]
        bad += [f"optimizer state of parameter {i} moved" for i, st in o0["state"].items()
                if not all(torch.equal(st[f], s1[i][f]) for f in ("step", "exp_avg", "exp_avg_sq"))]
    assert not bad and int(mod.engine.blk.step) == 0, "\n".join(bad[:20])


@pytest.mark.parametrize("zeroed", ["low", "high"])
def test_obs_embedding_gradient_is_the_sum_of_both_policies(zeroed):
    """The obs rows of the encoder's output gradient are the SUM of both policies' input gradients.  With one policy's first
    layer zeroed its input gradient vanishes, so the obs rows must equal the OTHER policy's contribution exactly - whichever
    policy is zeroed: an implementation that lets one contribution overwrite the other fails one of the two cases."""
    g = Golden("ril_twocam")
    mod = build(g)
    with torch.no_grad():
        mod.state_dict()[f"{zeroed}_level_policy.policy.fc_layers.0.weight"].zero_()
    _step(mod, U.golden_batch(g, 0))
    e = mod.engine
    B, other = e.B, "high" if zeroed == "low" else "low"
    assert float(e.dS[e.row0[zeroed]: e.row0[zeroed] + B].abs().max()) == 0.0
    for c in e.cams:
        j = e.order[other].index(c)
        want = e.dS[e.row0[other]: e.row0[other] + B, 32 * j: 32 * j + 32]
        got = e.enc_dout[c][:B]
        assert float(want.abs().max()) > 0 and torch.equal(got, want), (zeroed, c, (got - want).abs().max().item())
    # and with neither zeroed the rows are the sum
    mod = build(g)
    _step(mod, U.golden_batch(g, 0))
    e = mod.engine
    for c in e.cams:
        jl, jh = e.low_cams.index(c), e.high_cams.index(c)
        want = e.dS[:B, 32 * jl: 32 * jl + 32] + e.dS[B:, 32 * jh: 32 * jh + 32]
        assert torch.equal(e.enc_dout[c][:B], want)


def test_uint8_hwc_frames_equal_their_normalised_fp32_images():
    g = Golden("ril_twocam")
    u8, f32 = U.to_uint8_hwc(U.golden_batch(g, 0))
    a, b = build(g), build(g)
    la, lb = _step(a, u8), _step(b, f32)
    assert la == lb and all(torch.equal(a.engine.X3[c], b.engine.X3[c]) for c in a.engine.cams)
    assert torch.equal(a.engine.blk.param, b.engine.blk.param)


def test_two_rank_shards_equal_the_full_batch_step():
    """Two ranks (one GPU each, RCCL) on shards of 2 + 2 samples against one rank on B = 4 (tests/ril_shard_script.py)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "ril_shard_script.py")]
    out = run_group(cmd, env, ROOT, timeout=300)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_trainer_fit_smoke():
    """tacorl_amd.lightning.MiniTrainer drives two batches of the module in a fresh interpreter (tests/ril_fit_script.py)."""
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, env.get("PYTHONPATH", "")])
    out = run_group([sys.executable, os.path.join(ROOT, "tests", "ril_fit_script.py")], env, ROOT, timeout=240)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
