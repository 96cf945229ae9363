"""The logistic-mixture loss, backward and sample WITHOUT the gripper head (tacorl_logistic_mixture_nogrip_{loss, finish, sample},
reference action_decoder_logistic.py:52,134-138,184-235,238-266 with discrete_gripper: False - the D4RL decoder) against an
fp64 restatement of the reference's expressions written here, gradients by autograd on that fp64 graph.

Tolerances are those of the gripper variant's mixture term (tests/test_action_decoder_gpu.py RTOL / K_REF32, the elementwise
rule of tests/test_seq_gpu.py with the same term magnitudes): the per-dimension arithmetic is the same.  The inputs are chosen on
the CPU so that the restatement takes every branch of `_logistic_loss`; that is asserted from the restatement's own masks before
the kernel is looked at.  The gripper entry points, whose kernels became one template instantiation of the same source, are
called before and after the new ones in one process and must give the same bits."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_action_decoder_gpu import K_REF32, RTOL
from tests.test_seq_gpu import _check as _seq_check
from tests.test_seq_gpu import _dev, _exact, _L, _lm_case, _lm_scales, _nan, _rc, _untouched

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM = -22, -12
LOG_SIG_MIN = -5.0  # reference action_decoder_logistic.py:18


def _check(name, got, ref, ref32=None, scale=None):
    _seq_check(name, got, ref, ref32, scale=scale, rtol=RTOL, k=K_REF32)


def _views(h, B, Tm, Da, K):
    """Kernel heads rows (t B + b) -> the reference's (B, Tm, Da, K) means, log_scales, logit_probs."""
    n = Da * K
    hv = h.view(Tm, B, -1).transpose(0, 1)
    return tuple(hv[..., i * n:(i + 1) * n].reshape(B, Tm, Da, K) for i in range(3))


def _restate(h, act, B, Tm, Da, K, nc, dt, gs=1.0):
    """ActionDecoderLogistic._loss with discrete_gripper False (:134-138) = _logistic_loss (:184-235) on all Da dimensions,
    bounds +-1: (loss, d(gs loss)/d heads, the branch masks)."""
    n = Da * K
    h_ = h[:, :3 * n].to(dt).requires_grad_()
    mu, ls_raw, lg = _views(h_, B, Tm, Da, K)
    ls = torch.clamp(ls_raw, min=LOG_SIG_MIN)
    a = act[:, :Tm].to(dt).unsqueeze(-1) * torch.ones(1, 1, 1, K, dtype=dt)
    c, inv = a - mu, torch.exp(-ls)
    hb = 1.0 / (nc - 1)  # act_range / (num_classes - 1), act_range = (1 - -1) / 2
    plus_in, min_in, mid_in = inv * (c + hb), inv * (c - hb), inv * c
    cdf_delta = torch.sigmoid(plus_in) - torch.sigmoid(min_in)
    log_cdf_plus, log_one_minus_cdf_min = plus_in - F.softplus(plus_in), -F.softplus(min_in)
    log_pdf_mid = mid_in - ls - 2.0 * F.softplus(mid_in)
    lo, hi, wide = a < -1.0 + 1e-3, a > 1.0 - 1e-3, cdf_delta > 1e-5
    lp = torch.where(lo, log_cdf_plus, torch.where(hi, log_one_minus_cdf_min, torch.where(
        wide, torch.log(torch.clamp(cdf_delta, min=1e-12)), log_pdf_mid - math.log((nc - 1) / 2))))
    lp = lp + F.log_softmax(lg, dim=-1)
    loss = -torch.sum(torch.logsumexp(lp, dim=-1), dim=-1).mean()
    g, = torch.autograd.grad(loss * gs, h_)
    masks = {"x < -0.999": lo, "x > 0.999": hi & ~lo, "cdf_delta > 1e-5": wide & ~lo & ~hi, "mid-point": ~wide & ~lo & ~hi,
             "log_scale clamped": (ls_raw < LOG_SIG_MIN).detach()}
    return loss.detach(), g, masks


def _case(B, T, Tm, Da, K, nc, seed):
    """Heads [R][3 Da K + 5] (NaN padding) and actions [B][T][Da]: the mixture part of test_seq_gpu._lm_case, which places
    x = -1, -0.9995, 0.9995, 1, log-scales at and below the clamp, and tiny scales far from x (the mid-point branch), and keeps
    every element a factor e^0.5 away from the cdf_delta threshold so that fp32 and fp64 take the same branch."""
    hg, actg, _ = _lm_case(B, T, Tm, Da, K, nc, seed)
    n = Da * K
    h = torch.full((hg.shape[0], 3 * n + 5), float("nan"))
    h[:, :3 * n] = hg[:, :3 * n]
    return h, actg[..., :Da].contiguous(), (hg, actg)


# (B, T, Tm, Da, K, num_classes): the D4RL decoder's Da = 8 and a single dimension at the experiment's window (7 decoder steps);
# B Tm Da = 16 800 pairs > 1024 workgroups x 16: the grid-stride loop runs and every workgroup's partial sum is read
CASES = {"Da1": (3, 8, 7, 1, 10, 10), "Da8": (3, 8, 7, 8, 10, 10), "Da8_grid_stride": (300, 8, 7, 8, 10, 10)}


@pytest.mark.parametrize("case", list(CASES))
def test_nogrip_loss_and_backward(case):
    from tacorl_amd import ops

    B, T, Tm, Da, K, nc = CASES[case]
    R, n, gs = Tm * B, Da * K, 3.0
    h, act, (hg, actg) = _case(B, T, Tm, Da, K, nc, seed=R + K + Da)
    l64, g64, masks = _restate(h, act, B, Tm, Da, K, nc, torch.float64, gs)
    l32, g32, masks32 = _restate(h, act, B, Tm, Da, K, nc, torch.float32, gs)
    # the condition on the inputs: every branch taken by the restatement, and the same ones in fp32
    for k, m in masks.items():
        assert m.any(), f"no element takes the branch `{k}`"
        assert torch.equal(m, masks32[k]), f"fp32 and fp64 disagree on `{k}`"
    assert (h[:, n:2 * n] == LOG_SIG_MIN).any()
    assert (R * Da + 15) // 16 > 1  # more than one workgroup's partial sum

    dev = _dev()
    ldh = h.shape[1]
    hd, ad = h.to(dev), act.to(dev)
    nws = _L().lib().tacorl_logistic_mixture_ws_bytes(B, Tm, Da)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    dh = _nan(R, ldh, dev=dev)
    out, out_nograd, out_lazy = _nan(4, dev=dev), _nan(4, dev=dev), _nan(4, dev=dev)
    p, s = ops.ptr, ops.stream()
    args = (B, T, Tm, Da, K, nc, gs)
    ops.call("tacorl_logistic_mixture_nogrip_loss", p(hd), ldh, p(ad), p(dh), p(out), *args, p(ws), nws, s)
    ops.call("tacorl_logistic_mixture_nogrip_loss", p(hd), ldh, p(ad), None, p(out_nograd), *args, p(ws), nws, s)
    ops.call("tacorl_logistic_mixture_nogrip_loss", p(hd), ldh, p(ad), None, None, *args, p(ws), nws, s)
    ops.call("tacorl_logistic_mixture_nogrip_finish", p(ws), nws, B, Tm, Da, p(out_lazy), s)
    torch.cuda.synchronize()
    o = out.cpu()
    _untouched("out guard", o[2:])
    _exact("second output (no gripper accuracy)", o[1:2], torch.zeros(1))
    _exact("loss with d_heads NULL", out_nograd[:2], o[:2])
    _exact("loss by the lazy finish", out_lazy[:2], o[:2])
    _check("loss", o[0:1], l64.view(1), l32.view(1))
    d = dh.cpu()
    _untouched("d_heads padding", d[:, 3 * n:])
    below = h[:, n:2 * n] < LOG_SIG_MIN
    _exact("d log_scale below the clamp", d[:, n:2 * n][below], torch.zeros(int(below.sum())))
    assert (g64[:, n:2 * n][h[:, n:2 * n] == LOG_SIG_MIN] != 0).all()  # (at the bound the gradient passes)
    s_m, s_s, s_l = _lm_scales(hg, actg, B, Tm, Da, K, nc, gs)
    _check("d_heads means", d[:, :n], g64[:, :n], g32[:, :n], scale=s_m)
    _check("d_heads log_scales", d[:, n:2 * n][~below], g64[:, n:2 * n][~below], g32[:, n:2 * n][~below], scale=s_s[~below])
    _check("d_heads logit_probs", d[:, 2 * n:3 * n], g64[:, 2 * n:3 * n], g32[:, 2 * n:3 * n], scale=s_l)


def _sample_values(h, Da, K, ra, rb, dt):
    """_sample (:238-266) per component: the Gumbel scores (R, Da, K) and the value each component would give (R, Da, K)."""
    n = Da * K
    x = h[:, :3 * n].to(dt)
    mean, ls, lg = (x[:, i * n:(i + 1) * n].view(-1, Da, K) for i in range(3))
    ls = ls.clamp(min=LOG_SIG_MIN)  # (forward, :292)
    r1, r2 = 1e-5, 1.0 - 1e-5
    score = lg - torch.log(-torch.log((r1 - r2) * ra.to(dt) + r2))
    u = ((r1 - r2) * rb.to(dt) + r2).unsqueeze(-1)
    return score, mean + torch.exp(ls) * (torch.log(u) - torch.log(1.0 - u))


@pytest.mark.parametrize("R,Da", [(1, 1), (21, 8), (1025, 1), (40000, 8)])
def test_nogrip_sample(R, Da):
    """Injected uniforms: the component each output came from is the restatement's argmax, exactly, and the value is the
    restatement's within the kernel tolerance.  R Da = 320 000 > 1024 workgroups x 256: the grid-stride loop runs."""
    from tacorl_amd import ops

    K = 10
    n, ldh = Da * K, 3 * Da * K + 5
    g = torch.Generator().manual_seed(R + Da)
    h = torch.full((R, ldh), float("nan"))
    h[:, :n] = (torch.rand(R, n, generator=g) * 0.04 + 0.2 * torch.arange(K).repeat(Da) - 0.9)  # component means 0.2 apart
    h[:, n:2 * n] = torch.rand(R, n, generator=g) * 3 - 7  # log-scales in [-7, -4]: below and above the clamp, scales <= 0.02
    h[:, 2 * n:3 * n] = torch.randn(R, n, generator=g) * 2
    ra, rb = torch.rand(R, Da, K, generator=g), torch.rand(R, Da, generator=g) * 0.8 + 0.1  # |logit(u)| <= 2.2
    ra[0, 0, 0], ra[0, 0, K - 1] = 0.0, 1.0  # uniforms at the ends of [0, 1]
    # no near-tie of two Gumbel scores: where the restatement's margin is small, make its choice clear
    for _ in range(4):
        score, _ = _sample_values(h, Da, K, ra, rb, torch.float64)
        top = score.topk(2, -1)
        near = (top.values[..., 0] - top.values[..., 1]) < 1e-3
        if not near.any():
            break
        lgv = h[:, 2 * n:3 * n].view(R, Da, K)
        lgv[near] = lgv[near] + 0.5 * F.one_hot(top.indices[..., 0][near], K)
    score, val64 = _sample_values(h, Da, K, ra, rb, torch.float64)
    top = score.topk(2, -1)
    assert ((top.values[..., 0] - top.values[..., 1]) >= 1e-3).all()
    choice = top.indices[..., 0]
    _, val32 = _sample_values(h, Da, K, ra, rb, torch.float32)

    dev = _dev()
    T_ = [t.to(dev) for t in (h, ra, rb)]
    out = _nan(R * Da + 4, dev=dev)
    ops.call("tacorl_logistic_mixture_nogrip_sample", ops.ptr(T_[0]), ldh, ops.ptr(T_[1]), ops.ptr(T_[2]), ops.ptr(out), R, Da, K,
             ops.stream())
    torch.cuda.synchronize()
    o = out.cpu()
    _untouched("out guard", o[R * Da:])
    got = o[:R * Da].view(R, Da)
    assert torch.isfinite(got).all()
    # the components' values are >= 0.2 - 0.04 - 2 x 0.02 x 2.2 apart: the nearest one is the one the kernel chose
    implied = (got.double().unsqueeze(-1) - val64).abs().argmin(-1)
    _exact("mixture component", implied, choice)
    pick = lambda v: v.gather(-1, choice.unsqueeze(-1)).squeeze(-1)  # noqa: E731
    _check("actions", got, pick(val64), pick(val32))


def test_nogrip_refuses():
    """K = 17, a heads pitch narrower than 3 Da K, Tm > T: EINVAL; a workspace one byte short: ENOMEM; nothing written."""
    from tacorl_amd import ops

    dev = _dev()
    B, T, Tm, Da = 4, 5, 4, 2
    buf = torch.zeros(4096, device=dev)
    out, dh = _nan(4, dev=dev), _nan(4096, dev=dev)
    nws = _L().lib().tacorl_logistic_mixture_ws_bytes(B, Tm, Da)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    p, s = ops.ptr, ops.stream()
    loss = lambda ldh, T_, Tm_, K, nb: _rc("tacorl_logistic_mixture_nogrip_loss", p(buf), ldh, p(buf), p(dh), p(out), B, T_, Tm_, Da,  # noqa: E731
                                           K, 10, 1.0, p(ws), nb, s)
    assert loss(3 * Da * 17, T, Tm, 17, nws) == EINVAL
    assert loss(3 * Da * 10 - 1, T, Tm, 10, nws) == EINVAL
    assert loss(3 * Da * 10, T, T + 1, 10, nws) == EINVAL
    assert loss(3 * Da * 10, T, Tm, 10, nws - 1) == ENOMEM
    assert _rc("tacorl_logistic_mixture_nogrip_finish", p(ws), nws - 1, B, Tm, Da, p(out), s) == ENOMEM
    assert _rc("tacorl_logistic_mixture_nogrip_sample", p(buf), 3 * Da * 17, p(buf), p(buf), p(dh), 4, Da, 17, s) == EINVAL
    assert _rc("tacorl_logistic_mixture_nogrip_sample", p(buf), 3 * Da * 10 - 1, p(buf), p(buf), p(dh), 4, Da, 10, s) == EINVAL
    torch.cuda.synchronize()
    _untouched("loss", out)
    _untouched("d_heads / sample output", dh)


def test_gripper_entry_points_unmoved_by_the_new_ones():
    """tacorl_logistic_mixture_{loss, finish, sample} on one shape, then the no-gripper entry points on the same buffers' mixture
    part, then the gripper ones again: the same bits (loss, accuracy, every d_heads element, every sampled action)."""
    from tacorl_amd import ops

    dev = _dev()
    B, T, Tm, Da, K, nc = 9, 12, 11, 6, 10, 256
    R, n = Tm * B, Da * K
    h, act, ldh = _lm_case(B, T, Tm, Da, K, nc, seed=7)
    g = torch.Generator().manual_seed(3)
    ra, rb = torch.rand(R, Da, K, generator=g).to(dev), torch.rand(R, Da, generator=g).to(dev)
    hd, ad = h.to(dev), act.to(dev)
    nws = _L().lib().tacorl_logistic_mixture_ws_bytes(B, Tm, Da)
    p, s = ops.ptr, ops.stream()

    def gripper():
        ws = torch.zeros(nws, dtype=torch.uint8, device=dev)
        dh, out, lazy, smp = _nan(R, ldh, dev=dev), _nan(2, dev=dev), _nan(2, dev=dev), _nan(R, Da + 1, dev=dev)
        ops.call("tacorl_logistic_mixture_loss", p(hd), ldh, p(ad), p(dh), p(out), B, T, Tm, Da, K, nc, 0.5, 3.0, p(ws), nws, s)
        ops.call("tacorl_logistic_mixture_loss", p(hd), ldh, p(ad), None, None, B, T, Tm, Da, K, nc, 0.5, 3.0, p(ws), nws, s)
        ops.call("tacorl_logistic_mixture_finish", p(ws), nws, B, Tm, Da, p(lazy), s)
        ops.call("tacorl_logistic_mixture_sample", p(hd), ldh, p(ra), p(rb), p(smp), R, Da, K, s)
        torch.cuda.synchronize()
        return [t.cpu() for t in (dh, out, lazy, smp)]

    before = gripper()
    ws = torch.zeros(nws, dtype=torch.uint8, device=dev)
    act_ng = ad[..., :Da].contiguous()
    dh, out, smp = _nan(R, ldh, dev=dev), _nan(2, dev=dev), _nan(R, Da, dev=dev)
    ops.call("tacorl_logistic_mixture_nogrip_loss", p(hd), ldh, p(act_ng), p(dh), p(out), B, T, Tm, Da, K, nc, 3.0, p(ws), nws, s)
    ops.call("tacorl_logistic_mixture_nogrip_sample", p(hd), ldh, p(ra), p(rb), p(smp), R, Da, K, s)
    torch.cuda.synchronize()
    after = gripper()
    for name, a, b in zip(("d_heads", "loss / accuracy", "lazy loss / accuracy", "sample"), before, after):
        _exact(f"gripper {name}", b, a)
    assert torch.isfinite(before[1]).all() and torch.isfinite(before[3]).all()
    # and the two variants share the mixture arithmetic: the same mixture gradients and the same sampled actions, bit for bit
    _exact("mixture d_heads of the two variants", dh.cpu()[:, :3 * n], before[0][:, :3 * n])
    _exact("sampled actions of the two variants", smp.cpu(), before[3][:, :Da])
