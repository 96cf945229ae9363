"""Kernel-level tests of the small per-step kernels around the policy head, the plan distributions, alpha and the
optimiser: the batched tanh-Gaussian sampler, the actor head backward, actor_qmin, the alpha loss (and its fused Adam
step), the batched Adam with bf16 mirrors, the balanced Gaussian KL, the plan-recognition sample and its backward, the
logistic-mixture sampler and the uniform actions.

Every output is compared with an fp64 evaluation of the reference's own expressions (oracle/tacorl_oracle.py where it has
them), gradients by torch.autograd - never with the kernels' closed forms - at the edges where small kernels go wrong:
workgroup and grid-stride boundaries, clamp bounds hit exactly, ties, scalar tails, the width limits the launchers
enforce.  Outputs are filled with NaN (or a sentinel) first and have a leading dimension wider than their rows where
the ABI has one; elsewhere a guard tail behind the written range must keep its sentinel.

Tolerances, elementwise:  |got - ref64| <= RTOL * (|ref64| + median|ref64| of the block) + K_REF32 * |ref32 - ref64|
where ref32 is the same reference evaluated in fp32 (what the reference itself computes).  Clamp-masked gradient
entries, indices, +-1 gripper commands and outputs a comment claims are bit-identical are compared exactly."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM = -22, -12
F32_EPS = torch.finfo(torch.float32).eps
NAN = float("nan")
LG_ALPHA_LOSS, LG_ALPHA, LG_ACTOR_LOSS = 0, 1, 2
LG_COUNT = 18
# One fp32 evaluation of an elementwise expression (a handful of roundings and libm calls of a few ulp, 6e-8 each):
# 1e-5 leaves a margin of ~100x.  The median term gives elements that cancel to near zero (d log pi / d log_std =
# -1 + 2 a eps sd, a gradient that is the sum of terms of opposite sign) the absolute error of the terms they are made
# of, which are of the block's typical size.
RTOL = 1e-5
# Where the reference's own fp32 evaluation loses digits - z - mu at |mu| = 9 with sd = e^-5, 1 - u at u = 1 - 1e-5,
# the 0.999 clamp (0.999 in fp32 is not 0.999) - the kernel may lose as many, within a small multiple.
K_REF32 = 4.0


def _dev():
    from tacorl_amd import _lib

    _lib.call("tacorl_hip_init", 0)
    return torch.device("cuda:0")


def _L():
    from tacorl_amd import _lib

    return _lib


def _rc(name, *args):
    """Return code of a raw C-ABI call (the wrapper in _lib.call raises on anything but 0)."""
    return getattr(_L().lib(), name)(*args)


def _nan(*shape, dev):
    return torch.full(shape, NAN, device=dev)


def _check(name, got, ref, ref32=None, scale=None, rtol=RTOL, k=K_REF32):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{name}: {int((~torch.isfinite(got)).sum())} non-finite outputs"
    mag = (ref if scale is None else scale.detach().double().cpu()).abs()
    tol = rtol * (mag + mag.flatten().median())
    if ref32 is not None:
        tol = tol + k * (ref32.detach().double().cpu() - ref).abs()
    err = (got - ref).abs()
    worst = (err / tol.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print(f"tolerance-use {name}: {worst:.3g}")
    assert worst <= 1.0, f"{name}: worst error {worst:.3g} x its tolerance (max abs error {err.max().item():.3g})"


def _exact(name, got, ref):
    got, ref = got.detach().cpu(), ref.detach().cpu().to(got.dtype)
    bad = got != ref
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.numel()} differ, first at {bad.nonzero()[0].tolist()}: " \
                          f"{got[bad][0].item()} vs {ref[bad][0].item()}"


def _untouched(name, t):
    t = t.detach().cpu()
    ok = torch.isnan(t).all() if t.is_floating_point() else (t == -7).all()
    assert ok, f"{name}: padding / guard elements were written"


def _edge_heads(head, Ac):
    """Exact clamp bounds, values beyond them, the z - mu precision case, saturated tanh, tied gripper logits;
    rows taken modulo M so that every M gets some."""
    M = head.shape[0]
    cols = range(Ac)
    for r, mr, ls in ((0, 9.0, None), (1, -9.0, None), (2, 9.5, None), (3, -12.0, None), (4, 9.0, -5.0),
                      (5, -9.0, -5.0), (6, 9.0, 2.0), (7, None, 2.0), (8, None, -5.0), (9, None, -7.0),
                      (10, None, 3.0)):
        for j in cols:
            if (j + r) % 3 == 0 or r in (4, 5, 6):
                if mr is not None:
                    head[r % M, j] = mr
                if ls is not None:
                    head[r % M, Ac + j] = ls
    head[11 % M, 2 * Ac:2 * Ac + 2] = 0.75  # tied gripper logits
    head[12 % M, 2 * Ac:2 * Ac + 2] = torch.tensor([30.0, -30.0])


def _heads(M, Ac, ld, seed):
    g = torch.Generator().manual_seed(seed)
    h = torch.full((M, ld), NAN)
    h[:, :Ac] = (torch.rand(M, Ac, generator=g) * 2 - 1) * 4
    h[:, Ac:2 * Ac] = torch.rand(M, Ac, generator=g) * 4 - 3
    h[:, 2 * Ac:2 * Ac + 2] = torch.randn(M, 2, generator=g) * 2
    _edge_heads(h, Ac)
    return h


def _gumbel_u(n, M, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n, M, 2, generator=g)
    edge = torch.tensor([[0.0, 0.5], [1.0 - 2.0 ** -24, 0.3], [1.0, 0.7], [0.2, 1.0]])
    for r in range(4):
        u[:, r % M] = edge[r]
    u[:, 11 % M] = 0.4  # with the tied logits of row 11: an exact tie, the first index wins
    return u


# ============================================================================ tanh-Gaussian policy samples
def _policy_ref(head, Ac, eps, u, hard, dt, idx_override=None):
    """actor.py get_actions on a (M, HD) head: actions, log pi, the magnitude of log pi's terms, gripper index and
    the Gumbel-score margin of each row (0 on an exact tie, inf where a score is infinite)."""
    h = head.to(dt)
    mu = h[:, :Ac].clamp(-9.0, 9.0)
    sd = h[:, Ac:2 * Ac].clamp(-5.0, 2.0).exp()
    z = mu + eps.to(dt) * sd
    a, lp = torch.tanh(z), O_().tanh_logprob(z, mu, sd).squeeze(-1)
    terms = ((z - mu) ** 2 / (2 * sd * sd) + sd.log().abs() + 0.92 + 2 * (math.log(2) - z - F.softplus(-2 * z)).abs())
    scale = terms.sum(-1)
    idx = margin = None
    if u is not None:
        lg = h[:, 2 * Ac:2 * Ac + 2].expand(eps.shape[0], -1, -1)
        nl = lg - lg.logsumexp(-1, keepdim=True)
        if hard:  # RelaxedOneHotCategorical clamps u at the eps of the reference's dtype, fp32
            uu = u.clamp(F32_EPS, 1 - F32_EPS).to(dt)
            idx = O_().gumbel_rsample_hard_index(nl, uu)
        else:
            uu = u.to(dt)
            idx = O_().gumbel_argmax(nl, uu)
        s = nl - torch.log(-torch.log(uu))
        margin = (s[..., 1] - s[..., 0]).abs()
        if idx_override is not None:
            idx = idx_override
        glp = O_().gripper_logprob(lg, idx).squeeze(-1)
        lp, scale = lp + glp, scale + glp.abs()
        a = torch.cat([a, idx.unsqueeze(-1).to(dt) * 2 - 1], -1)
    return a, lp, scale, idx, margin


def O_():
    from oracle import tacorl_oracle as O

    return O


# (M, Ac, jobs [(head, n, gripper, hard_rsample, grip_idx pointer)], uniform job (u_rows, A, discrete) or None,
#  gumbel pointer array NULL)
SAMPLE_CASES = {
    "one_job_M63": (63, 16, [(0, 1, False, 0, False)], None, False),
    "step_dg_B256_n4": (256, 6, [(0, 1, True, 1, True), (1, 1, True, 0, False), (0, 4, True, 0, False),
                                 (1, 4, True, 0, False)], (4 * 256, 7, 1), False),
    # 2 x 32 x 1024 rows: twice the 2048 x 8 rows of one pass of the grid
    "step_B1024_n32_Ac16": (1024, 16, [(0, 1, False, 0, False), (1, 1, False, 0, False), (0, 32, False, 0, False),
                                       (1, 32, False, 0, False)], (32 * 1024, 16, 0), True),
    # six jobs, gripper / hard / grip_idx mixed per job; the uniform job needs more workgroups than any sampling job
    "six_jobs_Ac32_M65": (65, 32, [(0, 1, True, 1, True), (0, 2, True, 0, True), (1, 3, False, 0, False),
                                   (1, 1, True, 1, False), (0, 4, False, 0, False), (1, 2, True, 0, True)],
                          (3000, 33, 1), False),
    "Ac1_M257": (257, 1, [(0, 3, True, 1, True), (1, 2, False, 0, False)], (257, 2, 1), False),
    "M1": (1, 16, [(0, 1, True, 0, True), (0, 4, True, 1, True)], (1, 17, 1), False),
    "M255_no_gumbel_array": (255, 16, [(0, 2, False, 0, False), (1, 1, False, 0, False)], None, True),
    "dg_M1023": (1023, 6, [(0, 1, True, 1, True), (1, 1, True, 0, False), (0, 4, True, 0, True),
                           (1, 4, True, 0, False)], (4 * 1023, 7, 1), False),
    # 17 x 1025 = 17 425 rows > 16 384 (the grid-stride loop of the sampler runs) and 40 000 x 33 uniform elements
    # > 2048 x 256 (so does the uniform job's)
    "many_rows_Ac32": (1025, 32, [(0, 17, True, 1, True)], (40000, 33, 1), False),
}


def _uniform_u(rows, A, seed):
    u = torch.rand(rows, A, generator=torch.Generator().manual_seed(seed))
    for r, v in enumerate((0.5, 0.0, 1.0, 0.49999997, 0.50000006)[:rows]):  # u = 0.5 exactly gives 0 before the snap
        u[r, A - 1] = v
        u[r, 0] = v
    return u


def _uniform_ref(u, disc):
    """cql_offline_lightning.py:243-250 in fp32, as the reference computes it: 2u - 1 is two fp32 roundings at most
    (2u is exact), the same two the kernel does - compared bitwise."""
    v = u * 2.0 - 1.0
    if disc:
        v[:, -1] = torch.where(v[:, -1] >= 0, 1.0, -1.0)
    return v


@pytest.mark.parametrize("case", list(SAMPLE_CASES))
def test_tanh_normal_sample_batch(case):
    from tacorl_amd import ops

    dev = _dev()
    M, Ac, jobs, uni, null_gumbel = SAMPLE_CASES[case]
    HD, ld_head, ld_act = 2 * Ac + 2, 2 * Ac + 5, Ac + 5
    heads = [_heads(M, Ac, ld_head, seed=11 + i) for i in range(2)]
    heads_d = [h.to(dev) for h in heads]
    gen = torch.Generator().manual_seed(list(SAMPLE_CASES).index(case))
    J = []
    for ji, (hi, n, grip, hard, gptr) in enumerate(jobs):
        eps = torch.randn(n, M, Ac, generator=gen)
        eps[:, 6 % M] = 3.0  # mean 9 and sd e^2 in row 6: |z| > 10, tanh saturates
        eps[:, 3 % M, ::2] = -2.5
        u = _gumbel_u(n, M, seed=31 + ji) if grip else None
        J.append(dict(hi=hi, n=n, grip=grip, hard=hard, gptr=gptr, eps=eps, u=u, eps_d=eps.to(dev),
                      u_d=u.to(dev) if grip else None, act=_nan(n * M, ld_act, dev=dev), logp=_nan(n * M + 5, dev=dev),
                      gi=torch.full((n * M + 5,), -7, dtype=torch.int32, device=dev) if gptr else None))
    if uni:
        u_rows, A, disc = uni
        u01 = _uniform_u(u_rows, A, seed=5)
        u01_d, u_dst = u01.to(dev), _nan(u_rows, ld_act, dev=dev)
    else:
        u_rows, A, disc, u01_d, u_dst = 0, Ac + 1, 0, None, None
    gum = None if null_gumbel else ops.ptr_array([j["u_d"] for j in J])
    gia = ops.ptr_array([j["gi"] for j in J]) if any(j["gptr"] for j in J) else None
    ops.call("tacorl_tanh_normal_sample_batch", len(J), ops.ptr_array([heads_d[j["hi"]] for j in J]), ld_head,
             ops.ptr_array([j["eps_d"] for j in J]), gum, ops.int_array([j["hard"] for j in J]),
             ops.ptr_array([j["act"] for j in J]), ld_act, ops.ptr_array([j["logp"] for j in J]), gia,
             ops.int_array([j["n"] for j in J]), M, Ac, ops.ptr(u01_d), ops.ptr(u_dst), u_rows, A, disc, ops.stream())
    # the same draws through the one-thread-per-row kernel (rollout's)
    single = []
    for j in J:
        act1, lp1 = _nan(j["n"] * M, ld_act, dev=dev), _nan(j["n"] * M, dev=dev)
        gi1 = torch.full((j["n"] * M,), -7, dtype=torch.int32, device=dev)
        ops.tanh_normal_sample(heads_d[j["hi"]], ld_head, j["eps_d"], j["u_d"] if j["grip"] and not null_gumbel else None,
                               j["hard"], act1, 0, ld_act, lp1, gi1, j["n"], M, Ac)
        single.append((act1, lp1, gi1))
    torch.cuda.synchronize()

    for ji, j in enumerate(J):
        tag = f"{case}/job{ji}"
        n, grip = j["n"], j["grip"] and not null_gumbel
        Aj = Ac + (1 if grip else 0)
        head = heads[j["hi"]][:, :HD]
        a64, lp64, sc, idx64, margin = _policy_ref(head, Ac, j["eps"], j["u"] if grip else None, j["hard"], torch.float64)
        act = j["act"].cpu().view(n, M, ld_act)
        _untouched(f"{tag} act padding", act[..., Aj:])
        _untouched(f"{tag} logp guard", j["logp"][n * M:])
        idx_k = None
        if grip:
            idx_k = ((act[..., Ac] + 1) / 2).long()
            _exact(f"{tag} gripper command is +-1", act[..., Ac].abs(), torch.ones(n, M))
            # a near-tie of the two Gumbel scores (not an exact one: those must break to index 0 like torch.argmax) may
            # round either way in fp32; there the reference follows the kernel's index
            near = torch.isfinite(margin) & (margin > 0) & (margin < 1e-4)
            assert near.sum() <= max(2, n * M // 1000), f"{tag}: {int(near.sum())} near-tie rows"
            _exact(f"{tag} gripper index", idx_k[~near], idx64[~near])
            idx_use = torch.where(near, idx_k, idx64)
            a64, lp64, sc, _, _ = _policy_ref(head, Ac, j["eps"], j["u"], j["hard"], torch.float64, idx_use)
            a32, lp32, _, _, _ = _policy_ref(head, Ac, j["eps"], j["u"], j["hard"], torch.float32, idx_use)
            if j["gi"] is not None:
                _exact(f"{tag} grip_idx", j["gi"][:n * M].cpu().view(n, M), idx_k)
                _untouched(f"{tag} grip_idx guard", j["gi"][n * M:])
        else:
            a32, lp32, _, _, _ = _policy_ref(head, Ac, j["eps"], None, 0, torch.float32)
        _check(f"{tag} actions", act[..., :Ac], a64[..., :Ac], a32[..., :Ac])
        _check(f"{tag} log pi", j["logp"][:n * M].cpu().view(n, M), lp64, lp32, scale=sc)
        act1, lp1, gi1 = single[ji]
        # same expressions per element as the single kernel: bitwise; log pi differs in summation order only
        _exact(f"{tag} actions vs tacorl_tanh_normal_sample", j["act"][:, :Aj], act1[:, :Aj])
        _check(f"{tag} log pi vs tacorl_tanh_normal_sample", j["logp"][:n * M], lp1, scale=sc.flatten())
        if j["gi"] is not None:
            _exact(f"{tag} grip_idx vs tacorl_tanh_normal_sample", j["gi"][:n * M], gi1)
    if uni:
        got = u_dst.cpu()
        _exact(f"{case} uniform actions", got[:, :A], _uniform_ref(u01, disc))
        _untouched(f"{case} uniform padding", got[:, A:])


def test_tanh_normal_sample_batch_refuses_bad_shapes():
    from tacorl_amd import ops

    dev = _dev()
    M, Ac = 8, 33
    head, eps = torch.zeros(M, 2 * Ac + 2, device=dev), torch.zeros(M, Ac, device=dev)
    act, logp = _nan(M, Ac + 1, dev=dev), _nan(M, dev=dev)
    P = lambda t: ops.ptr_array([t] * 7)  # noqa: E731

    def run(njobs, ac):
        return _rc("tacorl_tanh_normal_sample_batch", njobs, P(head), 2 * Ac + 2, P(eps), None, ops.int_array([0] * 7),
                   P(act), Ac + 1, P(logp), None, ops.int_array([1] * 7), M, ac, None, None, 0, ac, 0, ops.stream())

    assert run(1, 33) == EINVAL
    assert run(0, 16) == EINVAL
    assert run(7, 16) == EINVAL
    assert run(6, 32) == 0  # the widest accepted
    torch.cuda.synchronize()
    assert torch.isfinite(act[:, :32]).all()


@pytest.mark.parametrize("rows,A,disc", [(1, 7, 1), (257, 7, 1), (1025, 16, 0), (300, 1, 1)])
def test_uniform_actions(rows, A, disc):
    from tacorl_amd import ops

    dev = _dev()
    u = _uniform_u(rows, A, seed=rows)
    ld = A + 3
    dst = _nan(rows, ld, dev=dev)
    ud = u.to(dev)
    ops.call("tacorl_uniform_actions", ops.ptr(ud), ops.ptr(dst), ld, rows, A, disc, ops.stream())
    torch.cuda.synchronize()
    got = dst.cpu()
    _exact("uniform actions", got[:, :A], _uniform_ref(u, disc))
    if disc:  # u = 0.5 exactly gives 0 before the snap: +1 (the reference's >= 0)
        assert got[0, A - 1].item() == 1.0
    _untouched("uniform padding", got[:, A:])


# ============================================================================ actor losses and head backward
def _qmin_ref(q1, q2, logp, la, gs, dt):
    q1, q2 = q1.to(dt).requires_grad_(), q2.to(dt).requires_grad_()
    alpha = la.to(dt).exp()[0]
    terms = alpha * logp.to(dt) - torch.min(q1, q2)  # cql_offline_lightning.py:463-466
    loss = terms.mean()
    g1, g2 = torch.autograd.grad(loss * gs, [q1, q2])
    return loss.detach(), g1, g2, alpha, terms.detach().abs().mean()


@pytest.mark.parametrize("B", [1, 63, 255, 257, 1025])
@pytest.mark.parametrize("ties", ["some", "all"])
def test_actor_qmin(B, ties):
    from tacorl_amd import ops

    dev = _dev()
    g = torch.Generator().manual_seed(B)
    q1, q2 = torch.randn(B, generator=g) * 5, torch.randn(B, generator=g) * 5
    if ties == "all":
        q2 = q1.clone()
    else:
        q2[::3] = q1[::3]
    logp = torch.randn(B, generator=g) * 4
    la = torch.tensor([-0.3])
    gs = 0.75
    T = [t.to(dev) for t in (q1, q2, logp, la)]
    dq1, dq2, logs = _nan(B + 4, dev=dev), _nan(B + 4, dev=dev), _nan(LG_COUNT + 4, dev=dev)
    ops.call("tacorl_actor_qmin", *[ops.ptr(t) for t in T[:3]], B, ops.ptr(T[3]), ops.ptr(dq1), ops.ptr(dq2), gs,
             ops.ptr(logs), ops.stream())
    torch.cuda.synchronize()
    loss64, g1, g2, alpha64, tsc = _qmin_ref(q1, q2, logp, la, gs, torch.float64)
    loss32, _, _, _, _ = _qmin_ref(q1, q2, logp, la, gs, torch.float32)
    # torch.min gives the whole gradient to the smaller one and splits a tie evenly; the zeros are exact, the rest is
    # one correctly rounded fp32 division -gs/B (and an exact halving): within 1 ulp
    for name, got, ref in (("dq1", dq1, g1), ("dq2", dq2, g2)):
        got = got.cpu()
        _exact(f"{name} zeros", got[:B][ref == 0], torch.zeros(int((ref == 0).sum())))
        _check(name, got[:B], ref, rtol=2.0 ** -23, k=0)
        _untouched(f"{name} guard", got[B:])
    lg = logs.cpu()
    # a mean over B fp32 terms: relative to the mean magnitude of the terms
    _check("actor_loss", lg[LG_ACTOR_LOSS:LG_ACTOR_LOSS + 1], loss64.view(1), loss32.view(1), scale=tsc.view(1))
    _check("alpha", lg[LG_ALPHA:LG_ALPHA + 1], alpha64.view(1), rtol=1e-6)  # one expf: a few ulp
    _untouched("other log slots", torch.cat([lg[:LG_ALPHA], lg[LG_ACTOR_LOSS + 1:]]))


def _critic(a, w, c, b):
    """A smooth stand-in critic Q(s, a) per row (the kernel only sees dQ/da): linear + quadratic in the action."""
    return (a * w).sum(-1) + 0.5 * (a * a * c).sum(-1) + b


def _actor_ref(head, eps, Ac, grip, idx, la, gs, mode, crit, value, logp, dt):
    """d(grad_scale * actor_loss)/d(raw head) through the reference's clamps and the rsample built from the same eps
    (cql_offline_lightning.py:439-468, actor.py:65-111), by autograd.  Q phase: the critic's gradient dQmin/da, split
    per critic as the engine's MLP backward delivers it, is what the kernel receives."""
    O = O_()
    h = head.to(dt).requires_grad_()
    mu = h[:, :Ac].clamp(O.MEAN_MIN, O.MEAN_MAX)
    sd = h[:, Ac:2 * Ac].clamp(O.LOG_SIG_MIN, O.LOG_SIG_MAX).exp()
    z = mu + eps.to(dt) * sd
    a, lpi = torch.tanh(z), O.tanh_logprob(z, mu, sd).squeeze(-1)
    logits = h[:, 2 * Ac:2 * Ac + 2]
    if grip:
        lpi = lpi + O.gripper_logprob(logits, idx).squeeze(-1)
    alpha = la.to(dt).exp()[0]
    out = {}
    if mode == "bc":
        lpd = O.tanh_logprob_of_value(value[:, :Ac].to(dt), mu, sd).squeeze(-1)
        if grip:
            lpd = lpd + O.gripper_logprob(logits, value[:, Ac].to(dt) / 2 + 0.5).squeeze(-1)
        loss = (alpha * lpi - lpd).mean()
        terms = alpha * logp.to(dt) - lpd  # the logged loss uses the sampled log pi the step passes in
        out["logged"], out["logged_scale"] = terms.mean().detach(), terms.abs().mean().detach()
    else:
        cs = [tuple(t.to(dt) for t in cr) for cr in crit]
        qmin = _critic(a, *cs[0]) if mode == "one" else torch.min(_critic(a, *cs[0]), _critic(a, *cs[1]))
        loss = (alpha * lpi - qmin).mean()
        # the per-critic action gradients of -gs * mean(Qmin), at the sampled action
        al = [a.detach().clone().requires_grad_() for _ in cs]
        qm = _critic(al[0], *cs[0]) if mode == "one" else torch.min(_critic(al[0], *cs[0]), _critic(al[1], *cs[1]))
        out["g_act"] = torch.autograd.grad(-qm.mean() * gs, al[:1] if mode == "one" else al)
    out["d_head"], = torch.autograd.grad(loss * gs, h)
    out["alpha"] = alpha.detach()
    return out


ACTOR_CASES = [  # (B, Ac, gripper, mode, grad_scale): B*Ac below, at and above the 1024 threads, and 8192
    (63, 6, True, "both", 1.0), (64, 16, False, "both", 1.0), (65, 16, False, "one", 0.5), (256, 32, False, "both", 0.25),
    (1024, 16, False, "both", 1.0), (1025, 6, True, "both", 1.0),
    (1, 16, False, "bc", 1.0), (63, 6, True, "bc", 1.0), (256, 16, False, "bc", 0.5), (1024, 6, True, "bc", 1.0),
    (256, 32, True, "bc", 1.0),
]


@pytest.mark.parametrize("B,Ac,grip,mode,gs", ACTOR_CASES)
def test_actor_head_bwd(B, Ac, grip, mode, gs):
    from tacorl_amd import ops

    dev = _dev()
    A, HD = Ac + (1 if grip else 0), 2 * Ac + (2 if grip else 0)
    ld_head, ld_g, ld_v = HD + 3, A + 4, A + 2
    head = _heads(B, Ac, ld_head, seed=B + Ac)
    if not grip:
        head[:, 2 * Ac:] = NAN
    g = torch.Generator().manual_seed(7 * B + Ac)
    eps = torch.randn(B, Ac, generator=g)
    eps[6 % B] = 3.0
    u = _gumbel_u(1, B, seed=B)[0]
    idx = _policy_ref(head[:, :HD], Ac, eps.unsqueeze(0), u.unsqueeze(0) if grip else None, 1,
                      torch.float64)[3] if grip else None
    idx = idx[0] if grip else None
    logp = torch.randn(B, generator=g) * 10
    la = torch.tensor([-0.7])
    crit = [(torch.randn(Ac, generator=g), torch.randn(Ac, generator=g), torch.randn(B, generator=g) * 2)
            for _ in range(2)]
    value = None
    if mode == "bc":
        value = torch.full((B, ld_v), NAN)
        value[:, :A] = torch.rand(B, A, generator=g) * 2 - 1
        for r, v in enumerate((1.0, -1.0, 0.9995, -0.9995, 0.999, -0.999, 0.0)):
            value[r % B, r % Ac] = v
        if grip:
            value[:, Ac] = torch.where(torch.rand(B, generator=g) < 0.5, -1.0, 1.0)
    ref = _actor_ref(head[:, :HD], eps, Ac, grip, idx, la, gs, mode, crit, value, logp, torch.float64)
    r32 = _actor_ref(head[:, :HD], eps, Ac, grip, idx, la, gs, mode, crit, value, logp, torch.float32)
    gact = [None, None]
    if mode != "bc":
        for i, ga in enumerate(ref["g_act"]):
            gact[i] = torch.randn(B, ld_g, generator=g) * 100  # the gripper column and the padding must be ignored
            gact[i][:, :Ac] = ga.float()
    T = {k: (v.to(dev) if v is not None else None) for k, v in dict(
        head=head, eps=eps, logp=logp, la=la, g1=gact[0], g2=gact[1], value=value,
        idx=idx.int() if grip else None).items()}
    d_head, logs = _nan(B, ld_head, dev=dev), _nan(LG_COUNT + 4, dev=dev)
    ops.call("tacorl_actor_head_bwd", ops.ptr(T["head"]), ld_head, ops.ptr(T["eps"]), ops.ptr(T["logp"]),
             ops.ptr(T["g1"]), ops.ptr(T["g2"]), ld_g, ops.ptr(T["value"]), ld_v, ops.ptr(T["idx"]), ops.ptr(T["la"]),
             gs, ops.ptr(d_head), B, Ac, int(grip), ops.ptr(logs), ops.stream())
    torch.cuda.synchronize()
    got = d_head.cpu()
    _untouched("d_head padding", got[:, HD:])
    raw = head[:, :2 * Ac]
    outside = torch.cat([(raw[:, :Ac] < -9) | (raw[:, :Ac] > 9), (raw[:, Ac:] < -5) | (raw[:, Ac:] > 2)], 1)
    at_bound = torch.cat([raw[:, :Ac].abs() == 9, (raw[:, Ac:] == -5) | (raw[:, Ac:] == 2)], 1)
    assert outside.any() and at_bound.any()
    # torch.clamp's gradient is exactly zero outside the bounds and passes at equality
    _exact("d_head beyond the clamps", got[:, :2 * Ac][outside], torch.zeros(int(outside.sum())))
    assert (got[:, :2 * Ac][at_bound] != 0).all() and (ref["d_head"][:, :2 * Ac][at_bound] != 0).all()
    _check("d_head mean", got[:, :Ac], ref["d_head"][:, :Ac], r32["d_head"][:, :Ac])
    _check("d_head log_std", got[:, Ac:2 * Ac], ref["d_head"][:, Ac:2 * Ac], r32["d_head"][:, Ac:2 * Ac])
    if grip:
        _check("d_head gripper logits", got[:, 2 * Ac:HD], ref["d_head"][:, 2 * Ac:HD], r32["d_head"][:, 2 * Ac:HD])
    lg = logs.cpu()
    if mode == "bc":
        _check("bc actor_loss", lg[LG_ACTOR_LOSS:LG_ACTOR_LOSS + 1], ref["logged"].view(1), r32["logged"].view(1),
               scale=ref["logged_scale"].view(1))
        _check("alpha", lg[LG_ALPHA:LG_ALPHA + 1], ref["alpha"].view(1), rtol=1e-6)  # one expf: a few ulp
    else:
        _untouched("logs (the Q phase logs in actor_qmin)", lg)


def _alpha_ref(logp, la, H, gs, dt):
    """cql_offline_lightning.py:447-449: alpha_loss = -mean(log_alpha * (logpi + target_entropy))."""
    la = la.to(dt).requires_grad_()
    t = logp.to(dt) + H
    loss = -(la[0] * t).mean()
    g, = torch.autograd.grad(loss * gs, la)
    return loss.detach(), g, t.abs().mean()


@pytest.mark.parametrize("B", [1, 255, 256, 257, 1024, 1025])
@pytest.mark.parametrize("gs", [1.0, 0.5])
def test_alpha_loss(B, gs):
    from tacorl_amd import ops

    dev = _dev()
    logp = torch.randn(B, generator=torch.Generator().manual_seed(B)) * 6 + 3
    la, H = torch.tensor([0.35]), -7.0
    ld, lad = logp.to(dev), la.to(dev)
    g, logs = _nan(2, dev=dev), _nan(LG_COUNT + 4, dev=dev)
    ops.call("tacorl_alpha_loss", ops.ptr(ld), B, ops.ptr(lad), H, gs, ops.ptr(g), ops.ptr(logs), ops.stream())
    torch.cuda.synchronize()
    l64, g64, sc = _alpha_ref(logp, la, H, gs, torch.float64)
    l32, g32, _ = _alpha_ref(logp, la, H, gs, torch.float32)
    # a mean over B fp32 terms: relative to the mean magnitude of the terms (times |log_alpha| for the loss)
    _check("g_log_alpha", g.cpu()[:1], g64, g32, scale=(sc * gs).view(1))
    _check("alpha_loss", logs.cpu()[LG_ALPHA_LOSS:1], l64.view(1), l32.view(1), scale=(sc * la.abs()).view(1))
    _untouched("g_log_alpha guard", g.cpu()[1:])
    _untouched("other log slots", logs.cpu()[1:])


@pytest.mark.parametrize("B", [1, 256, 1024, 1025])
def test_alpha_loss_step_equals_loss_then_adam(B):
    """rl_ops.hip: tacorl_alpha_loss_step is bit-identical to tacorl_alpha_loss + tacorl_adam_step(n = 1, max_norm = 0),
    the step counter advanced once per step, the loss logged with the pre-step log_alpha."""
    from tacorl_amd import ops

    dev = _dev()
    H, lr = -7.0, 3e-2
    la0 = torch.tensor([0.35])
    fused = [la0.clone().to(dev), torch.zeros(1, device=dev), torch.zeros(1, device=dev),
             torch.zeros(1, dtype=torch.int32, device=dev)]
    split = [t.clone() for t in fused]
    gf, gsp = _nan(1, dev=dev), _nan(1, dev=dev)
    lf, lsp = _nan(LG_COUNT, dev=dev), _nan(LG_COUNT, dev=dev)
    ws = torch.zeros(16, device=dev)
    P = {"log_alpha": la0.double().clone()}
    opt = O_().Adam(["log_alpha"], lr)
    for it in range(3):
        logp = torch.randn(B, generator=torch.Generator().manual_seed(10 * B + it)) * 6 + 3 + 4 * it
        ld = logp.to(dev)
        pre = fused[0].clone()
        ops.call("tacorl_alpha_loss_step", ops.ptr(ld), B, ops.ptr(fused[0]), H, ops.ptr(gf), ops.ptr(lf),
                 ops.ptr(fused[1]), ops.ptr(fused[2]), lr, ops.ptr(fused[3]), ops.stream())
        ops.call("tacorl_alpha_loss", ops.ptr(ld), B, ops.ptr(split[0]), H, 1.0, ops.ptr(gsp), ops.ptr(lsp), ops.stream())
        ops.call("tacorl_adam_step", ops.ptr(split[0]), ops.ptr(gsp), ops.ptr(split[1]), ops.ptr(split[2]), 1, lr, 0.0,
                 ops.ptr(split[3]), None, 0.0, ops.ptr(ws), ws.numel() * 4, ops.stream())
        torch.cuda.synchronize()
        for name, a, b in (("log_alpha", fused[0], split[0]), ("m", fused[1], split[1]), ("v", fused[2], split[2]),
                           ("step", fused[3], split[3]), ("g_log_alpha", gf, gsp), ("alpha_loss", lf[:1], lsp[:1])):
            _exact(f"step {it}: {name}", a, b)
        assert int(fused[3].item()) == it + 1
        l64, g64, sc = _alpha_ref(logp, pre.cpu(), H, 1.0, torch.float64)
        _check(f"step {it}: alpha_loss at the pre-step log_alpha", lf.cpu()[:1], l64.view(1),
               scale=(sc * pre.cpu().abs()).view(1))
        opt.step(P, {"log_alpha": g64})
        # fp64 Adam fed the fp64 gradient: the fp32 update's rounding of log_alpha and of the step, a few ulp of 0.35
        _check(f"step {it}: log_alpha vs fp64 Adam", fused[0].cpu(), P["log_alpha"], rtol=1e-6, k=0)


# ============================================================================ batched Adam with bf16 mirrors
BIG = 4 * 256 * 1024 + 5  # > 1024 workgroups of 256: the stride loop runs; n % 4 != 0: the scalar tail runs
# block: (n, offset in floats (1: 4 bytes off 16, the scalar path), Polyak target, max_norm, lr, mirror, target mirror)
ADAM_SPECS = {
    1: [(BIG, 0, True, 1.0, 3e-4, True, True)],
    4: [(1, 0, False, 0.0, 3e-4, True, False), (3, 0, True, 0.05, 1e-4, True, True),
        (257, 1, True, 1.0, 3e-4, True, True), (BIG, 0, False, 0.0, 3e-4, True, False)],
    8: [(1, 1, True, 0.0, 3e-4, False, False), (3, 0, False, 0.5, 3e-4, True, False),
        (257, 0, True, 0.0, 1e-4, True, True), (257, 1, False, 1.0, 3e-4, True, False),
        (1024, 0, True, 0.2, 3e-4, True, True), (1025, 0, True, 0.0, 3e-4, False, True),
        (BIG, 1, True, 0.0, 3e-4, True, True), (4096 + 7, 0, False, 2.0, 1e-4, True, False)],
}


def _adam_state(spec, dev, seed):
    g = torch.Generator().manual_seed(seed)
    S = []
    for bi, (n, off, has_t, mn, lr, mir, tmir) in enumerate(spec):
        def buf(fill=None):
            t = torch.empty(n + 8, device=dev)[off:off + n]
            t.copy_(fill if fill is not None else torch.zeros(n))
            return t

        S.append(dict(n=n, lr=lr, mn=mn, p=buf((torch.rand(n, generator=g) * 2 - 1)), m=buf(), v=buf(), g=buf(),
                      t=buf(torch.rand(n, generator=g) * 2 - 1) if has_t else None,
                      step=torch.zeros(1, dtype=torch.int32, device=dev),
                      mir=torch.empty(n + 8, dtype=torch.bfloat16, device=dev)[off:off + n] if mir else None,
                      tmir=torch.empty(n + 8, dtype=torch.bfloat16, device=dev)[off:off + n] if tmir and has_t else None))
    return S


def _adam_batch(S, ws):
    from tacorl_amd import ops

    k = len(S)
    arr = lambda key: ops.ptr_array([s[key] for s in S])  # noqa: E731
    return _rc("tacorl_adam_step_batch_mirror", k, arr("p"), arr("g"), arr("m"), arr("v"),
               (C.c_long * k)(*[s["n"] for s in S]), (C.c_float * k)(*[s["lr"] for s in S]),
               (C.c_float * k)(*[s["mn"] for s in S]), arr("step"), arr("t"),
               (C.c_float * k)(*[0.005 if s["t"] is not None else 0.0 for s in S]),
               arr("mir"), arr("tmir"), ops.ptr(ws), ws.numel(), ops.stream())


@pytest.mark.parametrize("nb", [1, 4, 8])
def test_adam_step_batch_mirror(nb):
    """include/tacorl_hip.h: tacorl_adam_step_batch(_mirror) is bit-identical to nb tacorl_adam_step calls; the mirrors
    are the updated parameters / targets in bf16."""
    from tacorl_amd import ops

    O = O_()
    dev = _dev()
    spec = ADAM_SPECS[nb]
    Sb, Ss = _adam_state(spec, dev, seed=nb), _adam_state(spec, dev, seed=nb)
    ws = torch.zeros(_L().lib().tacorl_adam_batch_ws_bytes(nb), dtype=torch.uint8, device=dev)
    ref = [dict(P={"w": sb["p"].cpu()}, t=sb["t"].cpu() if sb["t"] is not None else None, opt=O.Adam(["w"], sb["lr"]))
           for sb in Sb]
    for it in range(3):
        for bi, (sb, ss) in enumerate(zip(Sb, Ss)):
            gr = torch.randn(sb["n"], generator=torch.Generator().manual_seed(100 * it + bi)) * 0.01 * (it + 1)
            sb["g"].copy_(gr)
            ss["g"].copy_(gr)
            r = ref[bi]
            gd = {"w": gr.clone()}
            if sb["mn"] > 0:
                O.clip_grads_(gd, ["w"], sb["mn"])
            r["opt"].step(r["P"], gd)
            if r["t"] is not None:
                r["t"] = r["t"] * (1 - 0.005) + r["P"]["w"] * 0.005
        assert _adam_batch(Sb, ws) == 0
        for ss in Ss:
            wsz = _L().lib().tacorl_adam_ws_bytes(ss["n"])
            w1 = torch.zeros(max(wsz, 4), dtype=torch.uint8, device=dev)
            ops.call("tacorl_adam_step", ops.ptr(ss["p"]), ops.ptr(ss["g"]), ops.ptr(ss["m"]), ops.ptr(ss["v"]), ss["n"],
                     ss["lr"], ss["mn"], ops.ptr(ss["step"]), ops.ptr(ss["t"]), 0.005 if ss["t"] is not None else 0.0,
                     ops.ptr(w1), w1.numel(), ops.stream())
        torch.cuda.synchronize()
        for bi, (sb, ss) in enumerate(zip(Sb, Ss)):
            tag = f"step {it} block {bi} (n={sb['n']})"
            for key in ("p", "m", "v", "step", "t"):
                if sb[key] is not None:
                    _exact(f"{tag} {key} vs tacorl_adam_step", sb[key], ss[key])
            assert int(sb["step"].item()) == it + 1
            if sb["mir"] is not None:
                _exact(f"{tag} bf16 mirror", sb["mir"], sb["p"].to(torch.bfloat16))
            if sb["tmir"] is not None:
                _exact(f"{tag} bf16 target mirror", sb["tmir"], sb["t"].to(torch.bfloat16))
    for bi, sb in enumerate(Sb):
        # the tolerance of test_adam_clip_polyak: fp32 oracle and kernel differ in the norm's summation order and a
        # rounding or two per step (parameters in [-1, 1], lr <= 3e-4)
        r = ref[bi]
        assert (sb["p"].cpu() - r["P"]["w"]).abs().max().item() < 2e-7, f"block {bi}: param vs O.Adam"
        if sb["t"] is not None:
            assert (sb["t"].cpu() - r["t"]).abs().max().item() < 2e-7, f"block {bi}: target vs O.Adam"


def test_adam_step_batch_mirror_refuses():
    dev = _dev()
    spec = ADAM_SPECS[8] + [(5, 0, True, 0.0, 3e-4, True, True)]
    S = _adam_state(spec, dev, seed=3)
    ws9 = torch.zeros(_L().lib().tacorl_adam_batch_ws_bytes(9), dtype=torch.uint8, device=dev)
    assert _adam_batch(S, ws9) == EINVAL
    assert _adam_batch(S[:0], ws9) == EINVAL
    S4 = S[:4]
    need = _L().lib().tacorl_adam_batch_ws_bytes(4)
    assert _rc("tacorl_adam_batch_ws_bytes", 4) == need
    short = torch.zeros(need - 4, dtype=torch.uint8, device=dev)
    assert _adam_batch(S4, short) == ENOMEM
    odd = torch.empty(S4[2]["n"] + 8, dtype=torch.bfloat16, device=dev)
    S4[2]["mir"] = odd.data_ptr() + 1  # a bf16 mirror pointer at an odd byte address
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    p0 = [s["p"].clone() for s in S4]
    assert _adam_batch(S4, ws) == EINVAL
    torch.cuda.synchronize()
    for s, p in zip(S4, p0):  # refused before anything is launched
        assert int(s["step"].item()) == 0 and torch.equal(s["p"], p)


# ============================================================================ plan distributions
def _kl_ref(hq, hp, A, alpha, beta, min_std, balanced, gs, dt):
    """play_lmp_for_rl.py:259-301 on the raw heads: posterior std softplus(var_raw) + min_std, prior through the policy
    clamps; balanced: O.balanced_kl, else KL(q||p) with gradients to both."""
    O = O_()
    q, p = hq.to(dt).requires_grad_(), hp.to(dt).requires_grad_()
    mq, sq = q[:, :A], F.softplus(q[:, A:]) + min_std
    mp, sp = p[:, :A].clamp(O.MEAN_MIN, O.MEAN_MAX), p[:, A:].clamp(O.LOG_SIG_MIN, O.LOG_SIG_MAX).exp()
    if balanced:
        kl = O.balanced_kl(mq, sq, mp, sp, alpha)
    else:
        kl = torch.distributions.kl_divergence(torch.distributions.Normal(mq, sq),
                                               torch.distributions.Normal(mp, sp)).sum(-1).mean()
    dq, dp = torch.autograd.grad(beta * kl * gs, [q, p])
    vr = (sq / sp) ** 2
    scale = (0.5 * (vr + ((mq - mp) / sp) ** 2 + 1 + vr.log().abs())).sum(-1).mean()  # magnitude of the KL's terms
    return kl.detach(), dq, dp, scale.detach()


def _plan_heads(B, A, seed, prior):
    g = torch.Generator().manual_seed(seed)
    h = torch.empty(B, 2 * A)
    h[:, :A] = torch.randn(B, A, generator=g) * 2
    h[:, A:] = torch.randn(B, A, generator=g) * 2 - (1.0 if prior else 0.0)
    t20 = torch.tensor(20.0)
    up, dn = torch.nextafter(t20, t20 + 1).item(), torch.nextafter(t20, t20 - 1).item()  # fp32 neighbours of 20
    if prior:
        for r, (c, v) in enumerate(((0, 9.0), (1, -9.0), (2, 9.25), (3, -10.0), (A, -5.0), (A + 1, 2.0),
                                    (A + 2, -5.5), (A + 3 if A > 3 else A, 2.5))):
            h[r % B, c % (2 * A)] = v
    else:
        # softplus switches to the identity above 20 (fp32 neighbours of 20 on either side, and 20 itself)
        for r, v in enumerate((20.0, up, dn, 25.0, -12.0)):
            h[r % B, A + (r % A)] = v
    return h


@pytest.mark.parametrize("B,A", [(1, 16), (63, 16), (256, 16), (257, 16), (1025, 8)])
@pytest.mark.parametrize("balanced,alpha,gs", [(1, 0.8, 1.0), (1, 0.3, 0.5), (0, 0.8, 1.0)])
def test_gauss_kl_balanced(B, A, balanced, alpha, gs):
    from tacorl_amd import ops

    dev = _dev()
    beta, min_std = 1e-3, 1e-4
    hq, hp = _plan_heads(B, A, seed=B, prior=False), _plan_heads(B, A, seed=B + 1, prior=True)
    Tq, Tp = hq.to(dev), hp.to(dev)
    dq, dp, out = _nan(B * 2 * A + 8, dev=dev), _nan(B * 2 * A + 8, dev=dev), _nan(6, dev=dev)
    ops.call("tacorl_gauss_kl_balanced", ops.ptr(Tq), ops.ptr(Tp), ops.ptr(dq), ops.ptr(dp), B, A, alpha, beta, min_std,
             balanced, gs, ops.ptr(out), ops.stream())
    torch.cuda.synchronize()
    kl64, dq64, dp64, sc = _kl_ref(hq, hp, A, alpha, beta, min_std, balanced, gs, torch.float64)
    kl32, dq32, dp32, _ = _kl_ref(hq, hp, A, alpha, beta, min_std, balanced, gs, torch.float32)
    o = out.cpu()
    _check("kl", o[:1], kl64.view(1), kl32.view(1), scale=sc.view(1))
    _check("beta * kl", o[1:2], (beta * kl64).view(1), (beta * kl32).view(1), scale=(beta * sc).view(1))
    _untouched("out2 guard", o[2:])
    gq, gp = dq.cpu()[:B * 2 * A].view(B, 2 * A), dp.cpu()[:B * 2 * A].view(B, 2 * A)
    _untouched("d_head_q guard", dq.cpu()[B * 2 * A:])
    _untouched("d_head_p guard", dp.cpu()[B * 2 * A:])
    for name, got, r64, r32 in (("d_head_q mean", gq[:, :A], dq64[:, :A], dq32[:, :A]),
                                ("d_head_q var_raw", gq[:, A:], dq64[:, A:], dq32[:, A:]),
                                ("d_head_p mean", gp[:, :A], dp64[:, :A], dp32[:, :A]),
                                ("d_head_p log_std", gp[:, A:], dp64[:, A:], dp32[:, A:])):
        _check(name, got, r64, r32)
    outside = torch.cat([hp[:, :A].abs() > 9, (hp[:, A:] < -5) | (hp[:, A:] > 2)], 1)
    at_bound = torch.cat([hp[:, :A].abs() == 9, (hp[:, A:] == -5) | (hp[:, A:] == 2)], 1)
    _exact("d_head_p beyond the clamps", gp[outside], torch.zeros(int(outside.sum())))
    assert (gp[at_bound] != 0).all() and (dp64[at_bound] != 0).all()


def _pr_ref(head, eps, A, min_std, dt):
    """plan_recognition_transformer.py:100-104 and the TanhNormal rsample: tanh(mean + eps * (softplus(var) + min_std))."""
    h = head.to(dt).requires_grad_()
    mu, sd = h[:, :A], F.softplus(h[:, A:]) + min_std
    plan = torch.tanh(mu + eps.to(dt) * sd)
    return h, mu, sd, plan


@pytest.mark.parametrize("B,A", [(1, 16), (63, 16), (257, 32), (1025, 16)])
def test_pr_sample(B, A):
    from tacorl_amd import ops

    dev = _dev()
    min_std = 1e-4
    head = _plan_heads(B, A, seed=3 * B, prior=False)
    eps = torch.randn(B, A, generator=torch.Generator().manual_seed(B))
    _, mu64, sd64, pl64 = _pr_ref(head, eps, A, min_std, torch.float64)
    _, _, sd32, pl32 = _pr_ref(head, eps, A, min_std, torch.float32)
    hd, ed = head.to(dev), eps.to(dev)
    for drop in (None, "plan", "mu", "std"):
        outs = {k: _nan(B * A + 4, dev=dev) for k in ("plan", "mu", "std")}
        ops.call("tacorl_pr_sample", ops.ptr(hd), ops.ptr(ed), *[None if k == drop else ops.ptr(outs[k])
                                                                 for k in ("plan", "mu", "std")], B, A, min_std,
                 ops.stream())
        torch.cuda.synchronize()
        for k, t in outs.items():
            t = t.cpu()
            if k == drop:
                _untouched(f"{k} (NULL pointer given)", t)
                continue
            _untouched(f"{k} guard", t[B * A:])
            got = t[:B * A].view(B, A)
            if k == "mu":
                _exact("mu is the head's mean", got, head[:, :A])
            elif k == "std":
                _check("std", got, sd64.detach(), sd32.detach())
            else:
                _check("plan", got, pl64.detach(), pl32.detach())


@pytest.mark.parametrize("B,A", [(1, 16), (63, 16), (257, 32), (1025, 16)])
def test_pr_sample_bwd_accumulates(B, A):
    from tacorl_amd import ops

    dev = _dev()
    min_std = 1e-4
    head = _plan_heads(B, A, seed=5 * B, prior=False)
    g = torch.Generator().manual_seed(B + 1)
    eps, d_plan = torch.randn(B, A, generator=g), torch.randn(B, A, generator=g)
    d0 = torch.randn(B, 2 * A, generator=g)  # the KL's gradient already in d_head: the backward adds to it
    refs = {}
    for dt in (torch.float64, torch.float32):
        h, _, _, plan = _pr_ref(head, eps, A, min_std, dt)
        gr, = torch.autograd.grad((plan * d_plan.to(dt)).sum(), h)
        refs[dt] = (d0.to(dt) + gr, gr)
    dd = _nan(B * 2 * A + 4, dev=dev)
    dd[:B * 2 * A] = d0.flatten().to(dev)
    T = [t.to(dev) for t in (head, eps, d_plan)]
    ops.call("tacorl_pr_sample_bwd", *[ops.ptr(t) for t in T], ops.ptr(dd), B, A, min_std, ops.stream())
    torch.cuda.synchronize()
    got = dd.cpu()
    _untouched("d_head guard", got[B * 2 * A:])
    r64, gr64 = refs[torch.float64]
    # the sum of two terms: relative to both magnitudes
    _check("d_head", got[:B * 2 * A].view(B, 2 * A), r64, refs[torch.float32][0], scale=d0.abs() + gr64.abs())


# ============================================================================ logistic-mixture action sampler
def _lm_heads(R, Da, K, ldh, seed):
    g = torch.Generator().manual_seed(seed)
    h = torch.full((R, ldh), NAN)
    n = Da * K
    h[:, :n] = torch.randn(R, n, generator=g) * 0.5
    h[:, n:2 * n] = torch.rand(R, n, generator=g) * 5 - 7  # log-scales, many below LOG_SIG_MIN = -5
    h[:, 2 * n:3 * n] = torch.randn(R, n, generator=g) * 2
    h[:, 3 * n:3 * n + 2] = torch.randn(R, 2, generator=g)
    h[1 % R, 3 * n:3 * n + 2] = 0.25  # tied gripper logits: argmax takes the first, -1
    if K > 1:  # tied mixture logits (with tied rand_a below): tied Gumbel scores, the first maximum wins
        h[2 % R, 2 * n:2 * n + 2] = 1.5
    return h


def _lm_ref(h, Da, K, ra, rb, dt):
    """action_decoder_logistic.py:238-266 (log-scales clamped at LOG_SIG_MIN in forward, :292)."""
    O = O_()
    n = Da * K
    x = h.to(dt)
    mean = x[:, :n].view(-1, 1, Da, K)
    ls = x[:, n:2 * n].view(-1, 1, Da, K).clamp(min=O.LOG_SIG_MIN)
    lg = x[:, 2 * n:3 * n].view(-1, 1, Da, K)
    grip = x[:, 3 * n:3 * n + 2].view(-1, 1, 2)
    out = O.logistic_sample(lg, ls, mean, grip, ra.to(dt).view(-1, 1, Da, K), rb.to(dt).view(-1, 1, Da))[:, 0]
    r1, r2 = 1e-5, 1.0 - 1e-5
    t = lg - torch.log(-torch.log((r1 - r2) * ra.to(dt).view(-1, 1, Da, K) + r2))
    top = t.topk(min(2, K), -1).values[:, 0]
    margin = (top[..., 0] - top[..., 1]) if K > 1 else torch.full(top.shape[:-1], math.inf, dtype=dt)
    return out, margin


@pytest.mark.parametrize("R", [1, 63, 257, 1025])
@pytest.mark.parametrize("K", [1, 10, 16])
def test_logistic_mixture_sample(R, K):
    from tacorl_amd import ops

    dev = _dev()
    Da = 6
    ldh = 3 * Da * K + 2 + 5
    h = _lm_heads(R, Da, K, ldh, seed=R * K)
    g = torch.Generator().manual_seed(R + K)
    ra, rb = torch.rand(R, Da, K, generator=g), torch.rand(R, Da, generator=g)
    ra[2 % R, 0, :2] = 0.3
    for r, v in enumerate((0.0, 1.0)):  # uniforms at the ends of [0, 1]
        rb[r % R, r % Da] = v
        ra[(r + 3) % R, 1, r % K] = v
    T = [t.to(dev) for t in (h, ra, rb)]
    out = _nan(R * (Da + 1) + 4, dev=dev)
    ops.call("tacorl_logistic_mixture_sample", ops.ptr(T[0]), ldh, ops.ptr(T[1]), ops.ptr(T[2]), ops.ptr(out), R, Da, K,
             ops.stream())
    torch.cuda.synchronize()
    o = out.cpu()
    _untouched("out guard", o[R * (Da + 1):])
    got = o[:R * (Da + 1)].view(R, Da + 1)
    r64, margin = _lm_ref(h, Da, K, ra, rb, torch.float64)
    r32, _ = _lm_ref(h, Da, K, ra, rb, torch.float32)
    _exact("gripper command", got[:, Da], r64[:, Da])
    # a near-tie of two Gumbel scores (not an exact one) may pick either component in fp32: left out, and rare
    near = (margin > 0) & (margin < 1e-4)
    assert near.sum() <= max(2, R * Da // 500), int(near.sum())
    _check("actions", got[:, :Da][~near], r64[:, :Da][~near], r32[:, :Da][~near])


def test_logistic_mixture_sample_refuses_k17():
    from tacorl_amd import ops

    dev = _dev()
    buf = _nan(4096, dev=dev)
    assert _rc("tacorl_logistic_mixture_sample", ops.ptr(buf), 3 * 17 + 2, ops.ptr(buf), ops.ptr(buf), ops.ptr(buf), 4,
               1, 17, ops.stream()) == EINVAL
    torch.cuda.synchronize()
    _untouched("buffer", buf)
