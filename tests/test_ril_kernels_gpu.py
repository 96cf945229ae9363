"""Kernels added for relay imitation learning, against fp64 torch written here:

* tacorl_tanh_normal_nll - the behaviour-cloning loss of a tanh-Gaussian (+ discrete gripper) policy head and its gradient in
  one launch - held to the bound tests/test_heads_gpu.py holds tacorl_actor_head_bwd's `value` term to (same quantities):
  |got - ref64| <= RTOL (|ref64| + median |ref64|) + K_REF32 |ref32 - ref64|, clamp-masked gradients exactly zero;
* the TANH activation of the MLP kernels ([ReLU, ReLU, Tanh] goal encoders): forward, input and weight gradients - f32 mode
  at 1e-4 against fp64, bf16 mode (per-layer and fused kernels) against autograd with bf16 operand rounding at the
  tolerances tests/test_kernels_gpu.py uses for the MLP kernels."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_heads_gpu import NAN, _check, _dev, _exact, _heads, _nan, _untouched
from tests.test_kernels_gpu import FWD_BF16_ROUNDED, GRAD_BF16_ROUNDED, TOL_F32, relerr, rnd

pytestmark = pytest.mark.gpu
LOG2 = math.log(2.0)


def _nll_ref(head, target, Ac, grip, gs, dt):
    """-mean Actor.log_prob(target) (reference actor.py:140-156, utils/distributions.py:50-58, 86-109) and the gradient of
    gs * loss w.r.t. the raw head, by autograd."""
    h = head.to(dt).requires_grad_()
    mu = h[:, :Ac].clamp(-9.0, 9.0)
    sd = h[:, Ac:2 * Ac].clamp(-5.0, 2.0).exp()
    v = target[:, :Ac].to(dt).clamp(-0.999, 0.999)
    z = 0.5 * torch.log((1 + v).clamp(min=1e-6) / (1 - v).clamp(min=1e-6))
    lp = (-((z - mu) ** 2) / (2 * sd ** 2) - sd.log() - math.log(math.sqrt(2 * math.pi))).sum(-1)
    lp = lp + (-2.0 * (LOG2 - z - F.softplus(-2.0 * z))).sum(-1)
    if grip:
        idx = (target[:, Ac].to(dt) / 2 + 0.5).long()
        lp = lp + torch.gather(F.log_softmax(h[:, 2 * Ac:2 * Ac + 2], dim=-1), -1, idx.unsqueeze(-1)).squeeze(-1)
    loss = -lp.mean()
    d_head, = torch.autograd.grad(loss * gs, h)
    return loss.detach(), d_head, lp.detach().abs().mean()


@pytest.mark.parametrize("M,Ac,grip,gs", [(5, 32, False, 1.0), (5, 6, True, 1.0), (70, 32, False, 0.5), (70, 6, True, 0.5),
                                          (1, 6, True, 1.0), (67, 70, False, 1.0)])
def test_tanh_normal_nll(M, Ac, grip, gs):
    from tacorl_amd import ops

    dev = _dev()
    A, HD = Ac + (1 if grip else 0), 2 * Ac + (2 if grip else 0)
    ld_head, ld_t = HD + 3, A + 2
    head = _heads(M, Ac, ld_head, seed=M + Ac)  # raw means beyond +-9, log-stds beyond [-5, 2] and at the bounds, tied logits
    if not grip:
        head[:, 2 * Ac:] = NAN
    g = torch.Generator().manual_seed(11 * M + Ac)
    target = torch.full((M, ld_t), NAN)
    target[:, :A] = torch.rand(M, A, generator=g) * 2 - 1
    for r, v in enumerate((1.0, -1.0, 0.9995, -0.9995, 0.999, -0.999, 0.0)):
        target[r % M, r % Ac] = v
    if grip:
        target[:, Ac] = torch.where(torch.arange(M) % 2 == 0, -1.0, 1.0)  # both classes (one row: the first)
    ref = _nll_ref(head[:, :HD], target, Ac, grip, gs, torch.float64)
    r32 = _nll_ref(head[:, :HD], target, Ac, grip, gs, torch.float32)
    hd, td = head.to(dev), target.to(dev)
    d_head, logs = _nan(M, ld_head, dev=dev), _nan(4, dev=dev)
    ops.call("tacorl_tanh_normal_nll", ops.ptr(hd), ld_head, ops.ptr(td), ld_t, M, Ac, int(grip), gs, ops.ptr(d_head),
             ops._at(logs, 1), ops.stream())
    torch.cuda.synchronize()
    got, lg = d_head.cpu(), logs.cpu()
    _untouched("d_head padding", got[:, HD:])
    _untouched("log slots beside the written one", lg[[0, 2, 3]])
    raw = head[:, :2 * Ac]
    outside = torch.cat([(raw[:, :Ac] < -9) | (raw[:, :Ac] > 9), (raw[:, Ac:] < -5) | (raw[:, Ac:] > 2)], 1)
    if M >= 5:
        assert ((raw[:, :Ac] < -9) | (raw[:, :Ac] > 9)).any() and (raw[:, Ac:] < -5).any() and (raw[:, Ac:] > 2).any()
    # torch.clamp's gradient is exactly zero outside the bounds
    _exact("d_head beyond the clamps", got[:, :2 * Ac][outside], torch.zeros(int(outside.sum())))
    _check("d_head mean", got[:, :Ac], ref[1][:, :Ac], r32[1][:, :Ac])
    _check("d_head log_std", got[:, Ac:2 * Ac], ref[1][:, Ac:2 * Ac], r32[1][:, Ac:2 * Ac])
    if grip:
        _check("d_head gripper logits", got[:, 2 * Ac:HD], ref[1][:, 2 * Ac:HD], r32[1][:, 2 * Ac:HD])
    _check("nll", lg[1:2], ref[0].view(1), r32[0].view(1), scale=ref[2].view(1))
    # a second launch writes the same bits (the mean is a fixed-order sum)
    d2, l2 = _nan(M, ld_head, dev=dev), _nan(4, dev=dev)
    ops.call("tacorl_tanh_normal_nll", ops.ptr(hd), ld_head, ops.ptr(td), ld_t, M, Ac, int(grip), gs, ops.ptr(d2), ops._at(l2, 1),
             ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(l2[1], logs[1]) and torch.equal(d2[:, :HD], d_head[:, :HD])


def test_tanh_normal_nll_agrees_with_the_bc_term_of_actor_head_bwd():
    """The BC phase of CQL_Offline computes the same log-probability term inside tacorl_actor_head_bwd: with alpha's share
    removed (log_alpha = -inf -> alpha = 0) its gradient IS this kernel's, bit for bit, and its logged loss the same mean."""
    from tacorl_amd import ops

    dev = _dev()
    for M, Ac, grip in ((37, 6, True), (64, 32, False)):
        A, HD = Ac + (1 if grip else 0), 2 * Ac + (2 if grip else 0)
        head = _heads(M, Ac, HD + 2, seed=3 + M)[:, :HD].contiguous()
        g = torch.Generator().manual_seed(M)
        target = torch.rand(M, A, generator=g) * 2 - 1
        if grip:
            target[:, Ac] = torch.where(torch.rand(M, generator=g) < 0.5, -1.0, 1.0)
        hd, td = head.to(dev), target.to(dev)
        eps, logp = torch.zeros(M, Ac, device=dev), torch.zeros(M, device=dev)
        idx = torch.zeros(M, dtype=torch.int32, device=dev)
        la = torch.full((1,), float("-inf"), device=dev)
        d_a, logs_a = _nan(M, HD, dev=dev), _nan(22, dev=dev)
        ops.call("tacorl_actor_head_bwd", ops.ptr(hd), HD, ops.ptr(eps), ops.ptr(logp), None, None, 0, ops.ptr(td), A,
                 ops.ptr(idx) if grip else None, ops.ptr(la), 0.5, ops.ptr(d_a), M, Ac, int(grip), ops.ptr(logs_a), ops.stream())
        d_n, logs_n = _nan(M, HD, dev=dev), _nan(4, dev=dev)
        ops.call("tacorl_tanh_normal_nll", ops.ptr(hd), HD, ops.ptr(td), A, M, Ac, int(grip), 0.5, ops.ptr(d_n), ops.ptr(logs_n),
                 ops.stream())
        torch.cuda.synchronize()
        # (alpha = 0 leaves +-0 terms in actor_head_bwd's sums: x + 0 = x exactly)
        assert torch.equal(d_a, d_n), (d_a - d_n).abs().max().item()
        a, n = float(logs_a[2]), float(logs_n[0])  # LG_ACTOR_LOSS: the same terms, another summation order
        assert abs(a - n) <= 1e-5 * abs(n), (a, n)


MLP_CASES = [([32, 256, 256, 32], [1, 1, 3]), ([64, 256, 256, 32], [1, 1, 3]), ([32, 256, 32], [3, 3])]
MS = [5, 67]


def _act(h, a):
    return [h, F.relu(h), F.silu(h), torch.tanh(h)][a]


def _mlp_problem(i, M, dims, dev):
    from tacorl_amd import blocks

    L = len(dims) - 1
    Ws = [rnd(dims[l + 1], dims[l], seed=350 + i + l, scale=1 / math.sqrt(dims[l])) for l in range(L)]
    bs = [rnd(dims[l + 1], seed=360 + i + l, scale=0.1) for l in range(L)]
    x, dout = rnd(M, dims[0], seed=370 + i), rnd(M, dims[-1], seed=380 + i)
    flat = torch.zeros(blocks.mlp_size(dims), device=dev)
    v = blocks.mlp_views(flat, 0, dims, [(f"l{l}.w", f"l{l}.b") for l in range(L)])
    for l in range(L):
        v[f"l{l}.w"].copy_(Ws[l]); v[f"l{l}.b"].copy_(bs[l])
    return Ws, bs, x, dout, flat


def _autograd(Ws, bs, x, dout, acts, dt=torch.float64, rounded=False):
    from oracle import tacorl_oracle as O

    Ws, bs = [w.to(dt).requires_grad_() for w in Ws], [b.to(dt).requires_grad_() for b in bs]
    x = x.to(dt).requires_grad_()
    h = x
    for l, a in enumerate(acts):
        if rounded:
            with O.operand_rounding(torch.bfloat16):
                h = _act(O._linear(h, Ws[l], bs[l]), a)
        else:
            h = _act(F.linear(h, Ws[l], bs[l]), a)
    if rounded:
        with O.operand_rounding(torch.bfloat16):
            (h * dout.to(dt)).sum().backward()
    else:
        (h * dout.to(dt)).sum().backward()
    return h.detach(), x.grad, [w.grad for w in Ws], [b.grad for b in bs]


def _compare(tag, dims, acts, probs, actb, dxs, grads, refs, ftol, gtol):
    from tacorl_amd import blocks, ops

    L = len(dims) - 1
    for i, M in enumerate(MS):
        yo = ops.mlp_act_layout(M, dims, acts)[1][-1]
        y = actb[i][yo: yo + M * dims[-1]].view(M, dims[-1])
        errs = {"forward": (relerr(y, refs[i][0]), ftol), "dx": (relerr(dxs[i], refs[i][1]), gtol)}
        gv = blocks.mlp_views(grads[i], 0, dims, [(f"l{l}.w", f"l{l}.b") for l in range(L)])
        for l in range(L):
            errs[f"dW{l}"] = (relerr(gv[f"l{l}.w"], refs[i][2][l]), gtol)
            errs[f"db{l}"] = (relerr(gv[f"l{l}.b"], refs[i][3][l]), gtol)
        print(f"{tag} M={M}: " + ", ".join(f"{k} {e:.3g}" for k, (e, _) in errs.items()))
        bad = {k: e for k, (e, t) in errs.items() if not e < t}
        assert not bad, (tag, M, bad)


@pytest.mark.parametrize("dims,acts", MLP_CASES)
def test_mlp_tanh_f32(dims, acts):
    from tacorl_amd import ops

    dev = _dev()
    probs = [_mlp_problem(i, M, dims, dev) for i, M in enumerate(MS)]
    refs = [_autograd(*p[:4], acts) for p in probs]
    xs, douts, flats = [p[2].to(dev) for p in probs], [p[3].to(dev) for p in probs], [p[4] for p in probs]
    actb = [torch.zeros(ops.mlp_act_layout(M, dims, acts)[2], device=dev) for M in MS]
    grads, dxs = [torch.full_like(f, NAN) for f in flats], [_nan(M, dims[0], dev=dev) for M in MS]
    ops.mlp_fwd(xs, dims[0], flats, actb, MS, dims, acts, ops.F32)
    ops.mlp_bwd(xs, dims[0], flats, actb, douts, dims[-1], grads, dxs, dims[0], MS, dims, acts, ops.F32)
    torch.cuda.synchronize()
    _compare("f32", dims, acts, probs, actb, dxs, grads, refs, TOL_F32, TOL_F32)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("dims,acts", MLP_CASES)
def test_mlp_tanh_bf16(dims, acts, fused):
    """bf16 MFMA mode, per-layer kernels and the fused launches (what the goal encoder runs in bf16 mode), against
    autograd with the operands of every contraction rounded to bf16."""
    from tacorl_amd import ops

    dev = _dev()
    L = len(dims) - 1
    probs = [_mlp_problem(i, M, dims, dev) for i, M in enumerate(MS)]
    refs = [_autograd(*p[:4], acts, dt=torch.float32, rounded=True) for p in probs]
    xs, douts, flats = [p[2].to(dev) for p in probs], [p[3].to(dev) for p in probs], [p[4] for p in probs]
    actb = [torch.zeros(ops.mlp_act_layout(M, dims, acts)[2], device=dev) for M in MS]
    grads, dxs = [torch.zeros_like(f) for f in flats], [_nan(M, dims[0], dev=dev) for M in MS]
    if fused:
        assert ops.L.lib().tacorl_mlp_fwd_fused_supported(len(MS), L, ops.int_array(dims), dims[0]) == 1
        assert ops.mlp_bwd_fused_ok(len(MS), dims, dims[-1], dims[0], ops.BF16)
        fb = [f.to(torch.bfloat16) for f in flats]
        ops.mlp_fwd(xs, dims[0], flats, actb, MS, dims, acts, ops.BF16, params_bf16=fb)
        ops.mlp_bwd_fused_dgrad(flats, actb, douts, dims[-1], dxs, dims[0], MS, dims, acts, "t_ril_mlp")
        ops.mlp_bwd_fused_wgrad(xs, dims[0], actb, douts, dims[-1], grads, MS, dims, acts, "t_ril_mlp")
    else:
        ops.mlp_fwd(xs, dims[0], flats, actb, MS, dims, acts, ops.BF16)
        ops.mlp_bwd(xs, dims[0], flats, actb, douts, dims[-1], grads, dxs, dims[0], MS, dims, acts, ops.BF16)
    torch.cuda.synchronize()
    _compare("bf16 fused" if fused else "bf16 per-layer", dims, acts, probs, actb, dxs, grads, refs, FWD_BF16_ROUNDED,
             GRAD_BF16_ROUNDED)
