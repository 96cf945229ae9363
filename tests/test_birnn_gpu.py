"""The bidirectional-RNN plan recognition (`plan_recognition=tanh_net`, reference plan_encoders/plan_recognition_tanh_net.py)
on the GPU: the module's forward + backward against fp64 torch.nn.RNN, and the PlayLMP / TACORL steps that use it against
the reference's goldens (tools/gen_birnn_golden.py) and the oracle with the bi-RNN posterior (tests/test_birnn_cpu.py)."""
import copy

import pytest
import torch

from tests.golden_util import Golden, check_stats, gradient_floor, resync_oracle
from tests.test_birnn_cpu import TANH_NET, birnn_oracle  # noqa: F401  (fixture)
from tests.test_step_gpu import (ACTOR, CRITIC, GRAD_RTOL, PARAM_ATOL, RTOL, TACORL_YAML, _snap, check_logs,
                                 compare_with_oracle_grads, relerr, to_dev)

pytestmark = pytest.mark.gpu

NAN = float("nan")
H = 2048
# module level (test_seq_gpu.py's rule): |got - ref64| <= RTOL_MODULE * (|ref| + median |ref|) + K_REF32 * |ref32 - ref64|
RTOL_MODULE, K_REF32 = 1e-4, 4.0


def _dev():
    from tacorl_amd import _lib

    _lib.call("tacorl_hip_init", 0)
    return torch.device("cuda:0")


def _check(name, got, ref, ref32, T=None):
    """T: the rows are batch-major (b*T+t) and the median is taken per time step - the input gradient spans six orders of
    magnitude from t = T-1 back to t = 0 (the ReLU-RNN's gradient shrinks through every step), and a median over all of
    it would hold the last steps to a fraction of one fp32 rounding."""
    got, ref, ref32 = (t.detach().double().cpu() for t in (got, ref, ref32))
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{name}: {int((~torch.isfinite(got)).sum())} non-finite outputs"
    mag = ref.abs()
    if T is None:
        # (floored at 1e-3 of the largest magnitude: in a ReLU-sparse gradient the median is 0, which would hold a sum of a
        # few cancelling products to 1e-4 of its own small result)
        med = torch.maximum(mag.flatten().median(), 1e-3 * mag.max())
    else:
        m3 = mag.view(-1, T, mag.shape[-1])
        med = m3.transpose(0, 1).reshape(T, -1).median(dim=1).values.view(1, T, 1).expand_as(m3).reshape(mag.shape)
    tol = RTOL_MODULE * (mag + med) + K_REF32 * (ref32 - ref).abs()
    worst = ((got - ref).abs() / tol.clamp_min(1e-300)).max().item()
    print(f"tolerance-use {name}: {worst:.3g}")
    assert worst <= 1.0, f"{name}: worst error {worst:.3g} x its tolerance"


def _module(D, A, seed):
    from tacorl_amd.networks.plan_recognition_birnn import PlanRecognitionBiRNN
    from tacorl_amd.synth import param_values

    pr = PlanRecognitionBiRNN(state_dim=D, latent_plan_dim=A, device=_dev(), hidden_dim=H)
    with torch.no_grad():
        for k, v in pr.blk.views.items():
            v.copy_(param_values(k, v.shape, seed) * (3.0 if "bias" in k else 1.0))
    return pr


def _run(pr, emb, d_head, B, T, compute):
    """forward + backward with every output and gradient NaN-prefilled (an unwritten element fails the comparison)."""
    pr._ensure(B, T)
    pr.head.fill_(NAN)
    pr.blk.grad.fill_(NAN)
    if getattr(pr, "_bshape", (None, None))[:2] == (B, T):
        pr.dx.fill_(NAN)
    head = pr.forward(emb, emb.shape[1], B, T, compute).clone()
    dx = pr.backward(d_head, B, T, compute).clone()
    torch.cuda.synchronize()
    return head.cpu(), dx.cpu(), {k: v.detach().cpu().clone() for k, v in pr.blk.grad_views.items()}


def _gates(pr, B, T):
    """The module's own ReLU decisions (h > 0) of every state the output depends on: at B * T * 2H * 2 gates some
    pre-activations lie within fp32 rounding of zero, and a gate decided by the last bit there would move a whole batch
    row's gradient.  The reference takes these decisions and computes everything else itself (test_seq_gpu.py does the
    same for the transformer's ReLUs)."""
    H = pr.Hd
    y1 = pr.y1.detach().cpu().view(T + 2, B, 2 * H)[1:T + 1] > 0         # (T, B, 2H)
    y2 = pr.y2.detach().cpu().view(T + 1, B, H)[1:T] > 0                  # (T-1, B, H)
    h2 = pr.h2cat.detach().cpu() > 0                                       # (B, 2H)
    return y1, torch.cat([y2, h2[None, :, :H]], 0), h2[:, H:]


def _ref(P, emb, d_head, B, T, D, A, dtype, gates):
    """torch nn.RNN(relu, 2 layers, bidirectional, batch_first) + the heads as the reference defines them, restated with the
    given ReLU gates, autograd in `dtype` on the CPU."""
    g1, g2f, g2r = gates
    W = {k: v.to(dtype).clone().requires_grad_(True) for k, v in P.items()}
    lin = lambda x, n: x @ W[n + ".weight" if n.endswith("fc") else n].T  # noqa: E731
    x = emb.to(dtype).view(B, T, D).clone().requires_grad_(True)
    m = "birnn_model.{}_l{}{}"

    def cell(xt, h, l, sfx, gate):
        z = xt @ W[m.format("weight_ih", l, sfx)].T + W[m.format("bias_ih", l, sfx)]
        if h is not None:
            z = z + h @ W[m.format("weight_hh", l, sfx)].T
        return (z + W[m.format("bias_hh", l, sfx)]) * gate.to(dtype)

    f, r = [None] * T, [None] * T
    for t in range(T):
        f[t] = cell(x[:, t], f[t - 1] if t else None, 0, "", g1[t, :, :H])
    for t in reversed(range(T)):
        r[t] = cell(x[:, t], r[t + 1] if t < T - 1 else None, 0, "_reverse", g1[t, :, H:])
    y1 = [torch.cat([f[t], r[t]], -1) for t in range(T)]
    h = None
    for t in range(T):
        h = cell(y1[t], h, 1, "", g2f[t])
    hr = cell(y1[T - 1], None, 1, "_reverse", g2r)
    y = torch.cat([h, hr], -1)
    head = torch.cat([lin(y, "mean_fc") + W["mean_fc.bias"], lin(y, "variance_fc") + W["variance_fc.bias"]], -1)
    (head * d_head.to(dtype)).sum().backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in W.items()}
    return head.detach(), x.grad.reshape(B * T, D), grads


@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("T", [16, 32])
@pytest.mark.parametrize("B", [3, 32, 256])
def test_birnn_module_f32_vs_fp64(B, T, D):
    """Head, input gradient and every parameter gradient (by reference name) of the f32 path against fp64 autograd of the
    reference's nn.RNN (with the module's own ReLU decisions, _gates); weight_hh_l1_reverse's gradient is exactly zero (it only
    ever multiplies the zero state)."""
    dev = _dev()
    A = 16 if D == 32 else 32
    pr = _module(D, A, seed=B + T + D)
    g = torch.Generator().manual_seed(B * T + D)
    emb = torch.randn(B * T, D, generator=g)
    d_head = torch.randn(B, 2 * A, generator=g)
    head, dx, grads = _run(pr, emb.to(dev), d_head.to(dev), B, T, 0)
    P = {k: v.detach().cpu().clone() for k, v in pr.blk.views.items()}
    gates = _gates(pr, B, T)
    h64, dx64, g64 = _ref(P, emb, d_head, B, T, D, A, torch.float64, gates)
    h32, dx32, g32 = _ref(P, emb, d_head, B, T, D, A, torch.float32, gates)
    tag = f"B{B}/T{T}/D{D}"
    _check(f"{tag} head", head, h64, h32)
    _check(f"{tag} dx", dx, dx64, dx32, T=T)
    assert float(grads["birnn_model.weight_hh_l1_reverse"].abs().max()) == 0.0
    for k, gr in g64.items():
        _check(f"{tag} d {k}", grads[k], gr, g32[k])


def test_birnn_module_generic_shapes_f32_vs_fp64():
    """A hidden / latent width the ring GEMM and the stacked heads do not take (H 35, A 5: odd widths, the heads' two
    matrices are not adjacent in the block) runs the generic path - forward and backward against fp64 nn.RNN."""
    from tacorl_amd.networks.plan_recognition_birnn import PlanRecognitionBiRNN
    from tacorl_amd.synth import param_values

    global H
    dev, B, T, D, A, keep = _dev(), 5, 7, 32, 5, H
    H = 35
    try:
        pr = PlanRecognitionBiRNN(state_dim=D, latent_plan_dim=A, device=dev, hidden_dim=H)
        assert not pr._heads_stacked and not pr._ring_ok(B, T, 1)
        with torch.no_grad():
            for k, v in pr.blk.views.items():
                v.copy_(param_values(k, v.shape, 5) * (3.0 if "bias" in k else 1.0))
        g = torch.Generator().manual_seed(6)
        emb, d_head = torch.randn(B * T, D, generator=g), torch.randn(B, 2 * A, generator=g)
        for compute in (0, 1):  # (bf16 here: the generic GEMMs at bf16 operands; f32 checked against fp64)
            head, dx, grads = _run(pr, emb.to(dev), d_head.to(dev), B, T, compute)
            assert torch.isfinite(head).all() and torch.isfinite(dx).all()
        head, dx, grads = _run(pr, emb.to(dev), d_head.to(dev), B, T, 0)
        P = {k: v.detach().cpu().clone() for k, v in pr.blk.views.items()}
        gates = _gates(pr, B, T)
        h64, dx64, g64 = _ref(P, emb, d_head, B, T, D, A, torch.float64, gates)
        h32, dx32, g32 = _ref(P, emb, d_head, B, T, D, A, torch.float32, gates)
        _check("H35 head", head, h64, h32)
        _check("H35 dx", dx, dx64, dx32, T=T)
        for k, gr in g64.items():
            _check(f"H35 d {k}", grads[k], gr, g32[k])
    finally:
        H = keep


@pytest.mark.parametrize("T,D", [(16, 32), (32, 64)])
@pytest.mark.parametrize("B", [3, 32, 256])
def test_birnn_module_bf16_vs_rounded_restatement(B, T, D):
    """bf16 - the ring-GEMM path (tacorl_rnn_linear_ld, tacorl_rnn_wgrad(_batch) where R % 64 == 0) - against the fp32
    restatement of the posterior (tests/test_birnn_cpu.py) with the oracle's bf16 operand rounding: head to 2e-3, input
    gradient to 5e-2 (the end of 2T + 2 dependent bf16 contractions through ReLU gates that bf16 rounding flips differently
    on both sides: measured 1.0e-3 - 3.7e-2 over the grid), parameter gradients to 6e-2 (the same gate decisions summed over
    all T B rows: measured up to 4.1e-2, layer 1's input weights at B 256; relative norms).  The full-size
    steps (tests/test_birnn_fullsize_gpu.py) hold the same path to the rounded oracle with reproducibility floors."""
    from oracle import tacorl_oracle as O
    from tests.test_birnn_cpu import birnn_posterior

    dev = _dev()
    A = 16 if D == 32 else 32
    pr = _module(D, A, seed=7 + B + T)
    assert pr._ring_ok(B, T, 1)
    g = torch.Generator().manual_seed(8 + B)
    emb = torch.randn(B * T, D, generator=g)
    d_head = torch.randn(B, 2 * A, generator=g)
    head, dx, grads = _run(pr, emb.to(dev), d_head.to(dev), B, T, 1)
    assert pr._ringed
    P = {"plan_recognition." + k: v.detach().cpu().clone().requires_grad_(True) for k, v in pr.blk.views.items()}
    x = emb.view(B, T, D).clone().requires_grad_(True)
    y = _restated_last_hidden(P, x)  # [h2f_{T-1} | h2r_{T-1}]; the head is [mean | var_raw] of it
    with O.operand_rounding(torch.bfloat16):
        ref_head = torch.cat([O._linear(y, P["plan_recognition.mean_fc.weight"], P["plan_recognition.mean_fc.bias"]),
                              O._linear(y, P["plan_recognition.variance_fc.weight"], P["plan_recognition.variance_fc.bias"])],
                             dim=-1)
        mean, _ = birnn_posterior(P, "plan_recognition.", x)
    assert relerr(ref_head[:, :A], mean) < 1e-6
    (ref_head * d_head).sum().backward()
    print(f"bf16 B{B}/T{T}/D{D}: head relerr {relerr(head, ref_head):.3g}, dx {relerr(dx, x.grad.reshape(B * T, D)):.3g}")
    assert relerr(head, ref_head) < 2e-3, relerr(head, ref_head)
    assert relerr(dx, x.grad.reshape(B * T, D)) < 5e-2, relerr(dx, x.grad.reshape(B * T, D))
    for k, p in P.items():
        name = k[len("plan_recognition."):]
        if name == "birnn_model.weight_hh_l1_reverse":
            assert float(grads[name].abs().max()) == 0.0
            continue
        e = relerr(grads[name], p.grad)
        print(f"bf16 B{B}/T{T}/D{D} d {name}: relerr {e:.3g}")
        assert e < 6e-2, (name, e)


def _restated_last_hidden(P, x):
    """[h2f_{T-1} | h2r_{T-1}] of the restatement, under bf16 operand rounding."""
    from oracle import tacorl_oracle as O
    from tests.test_birnn_cpu import _rnn_direction

    T = x.shape[1]
    m = "plan_recognition.birnn_model.{}"
    with O.operand_rounding(torch.bfloat16):
        f1 = _rnn_direction(P, m + "_l0", x, range(T))
        r1 = _rnn_direction(P, m + "_l0_reverse", x, reversed(range(T)))
        y1 = torch.stack([torch.cat([f1[t], r1[t]], dim=-1) for t in range(T)], dim=1)
        f2 = _rnn_direction(P, m + "_l1", y1, range(T))[T - 1]
        r2 = _rnn_direction(P, m + "_l1_reverse", y1[:, T - 1:], [0])[0]
    return torch.cat([f2, r2], dim=-1)


# ------------------------------------------------------------------------------------------- steps
AD = dict(n_mixtures=10, num_layers=2, hidden_size=2048, out_features=7, num_classes=10, rnn_model="rnn_decoder",
          include_goal=False)


def _playlmp(g, compute="f32"):
    from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP

    cams, c = sorted(g.cams), g.cfg
    return PlayLMP(plan_proposal=ACTOR, plan_recognition=dict(TANH_NET, latent_plan_dim=c["latent"]),
                   action_decoder=dict(AD, latent_plan_dim=c["latent"]), plan_proposal_obs_modalities=cams,
                   plan_proposal_goal_modalities=cams, plan_recognition_modalities=cams, action_decoder_modalities=cams,
                   real_world=True, lr=1e-4, kl_beta=1e-3, device="cuda:0", compute_dtype=compute, image_dtype=compute)


def _tacorl(g, compute="f32"):
    from tacorl_amd.modules.tacorl.tacorl import TACORL

    c = g.cfg
    return TACORL(play_lmp=_playlmp(g, compute), finetune_action_decoder=c.get("finetune_ad", False), critic=CRITIC,
                  real_world=True, device="cuda:0", compute_dtype=compute, image_dtype=compute, **TACORL_YAML)


def test_playlmp_birnn_step(birnn_oracle):  # noqa: F811
    O = birnn_oracle
    g = Golden("playlmp_birnn")
    cams, c = sorted(g.cams), g.cfg
    mod = _playlmp(g)
    assert sorted(n for n, _ in mod.named_parameters()) == sorted(g.names)
    mod.load_state_dict(g.params(), strict=False)
    P = O.require_grad_(g.params())
    opt = O.Adam([n for n in P], 1e-4)
    for step in range(c["steps"]):
        batch, nz = g.batch(step), g.noise(step)
        if step:
            resync_oracle(mod, P, opt)
        mod.logged = {}
        mod.training_step(to_dev(batch, mod.device), 0, noise={k: nz[k] for k in ("eps_plan", "u_plan")})
        torch.cuda.synchronize()
        got = {k.split("/", 1)[1]: v for k, v in mod.logged.items()}
        before, opt0 = _snap(P), copy.deepcopy(opt)
        _, ograds = O.playlmp_step(P, opt, batch, nz, cams)
        floor = gradient_floor(lambda Pp: O.playlmp_step(Pp, copy.deepcopy(opt0), batch, nz, cams)[1], before, ograds)
        bad = check_logs(got, g.logged(step))
        bad += compare_with_oracle_grads(mod, ograds, GRAD_RTOL, floor)
        if step == 0:
            bad += check_stats(mod.named_gradients(), g.stats(step, "grad"), rtol=GRAD_RTOL, what="golden grad ")
        bad += check_stats(mod.state_dict(), g.stats(step, "param"), rtol=RTOL, atol=PARAM_ATOL if step == 0 else 2e-4,
                           what="golden param ")
        assert not bad, f"step {step}:\n" + "\n".join(bad[:25])


def test_tacorl_birnn_step_eager_and_graph(birnn_oracle):  # noqa: F811
    """Latent plans at 1e-4 and every logged scalar against the reference (eager), and the captured-graph step equal to
    the eager one over three steps (the third replays the graph)."""
    g = Golden("tacorl_birnn_q")
    mods = [_tacorl(g), _tacorl(g)]
    for m in mods:
        m.load_state_dict(g.params(), strict=False)
        m.current_epoch = g.cfg["epoch"]
    mods[1].enable_graph()
    for step in range(3):
        b, nz = g.batch(min(step, 1)), g.noise(min(step, 1))
        outs = []
        for m in mods:
            m.logged = {}
            m.training_step(to_dev(b, m.device), noise=to_dev(nz, m.device))
            torch.cuda.synchronize()
            outs.append({k.split("/", 1)[1]: v for k, v in m.logged.items()})
        if step < g.cfg["steps"]:
            bad = check_logs(outs[0], g.logged(step))
            e = relerr(mods[0].plan, g.latent_plan(step))
            assert e < RTOL, f"step {step}: latent plan relerr {e:.3g}"
            assert not bad, f"step {step}:\n" + "\n".join(bad[:25])
        diff = [f"{k}: graph {outs[1][k]:.9g} eager {v:.9g}" for k, v in outs[0].items()
                if abs(outs[1][k] - v) > 1e-6 * max(abs(v), 1e-2)]
        assert not diff, f"step {step}:\n" + "\n".join(diff)
        assert torch.equal(mods[0].plan, mods[1].plan), step
    assert len(mods[1]._graphs) == 1


def test_tacorl_birnn_validation_step():
    from tests.test_step_gpu import L_as_list

    g = Golden("val_tacorl_birnn")
    mod = _tacorl(g)
    mod.load_state_dict(g.params(), strict=False)
    mod.current_epoch = g.cfg["epoch"]
    mod.eval()
    before = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    opt_before = [o.state_dict() for o in L_as_list(mod.configure_optimizers())]
    mod.logged = {}
    mod.validation_step(to_dev(g.batch(0), mod.device), 0, noise=to_dev(g.noise(0), mod.device))
    torch.cuda.synchronize()
    got = {k.split("/", 1)[1]: v for k, v in mod.logged.items()}
    bad = check_logs(got, g.logged(0))
    assert not bad, "\n".join(bad)
    assert relerr(mod.plan, g.latent_plan(0)) < RTOL
    after = mod.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    for a, b in zip(opt_before, [o.state_dict() for o in L_as_list(mod.configure_optimizers())]):
        assert str(a) == str(b)
