"""Kernel-level test of tacorl_cql_loss (csrc/rl_ops.hip: cql_loss_kernel + cql_finish_kernel), the fused Bellman + CQL
log-sum-exp (+ Lagrange) loss that produces the critics' whole gradient in CQL_Offline and TACORL.

The reference is the reference module's own expressions (cql_offline_lightning.py:284-314, 357-398) in fp64, dq by
torch.autograd - never the kernel's closed forms - and the same in fp32 (`ref32`, what the reference itself computes).
Cases cross the batch sizes at which the kernel changes its path (B = 1: three waves of the only workgroup write zero
partials; B = 1027 > 1024: every wave walks more than one sample and all 256 workgroups run), the sample counts around
the one-lane / two-slot boundary (3n = 63 / 66) and the widest accepted (3n = 126), scalars that all differ from 1 and
from each other, `reward` and `done` as different tensors, both backups, the Lagrange weight absent, ordinary, tiny and
clamped at 1e6, a tie row and rows of large logits.

Tolerances are test_heads_gpu's rule, elementwise:
    |got - ref64| <= RTOL * (|ref64| + median|ref64| of the block) + K_REF32 * |ref32 - ref64|
dq in two blocks (data rows, sampled rows); for a logged scalar the median is replaced by the mean |summand| of that
scalar, from the fp64 reference.

Large logits.  A softmax entry e_j / sum(e) carries the relative error of e_j = exp(lg_j - max), that is the ABSOLUTE
error of lg_j = (q - sub) / temp: half an ulp of |q - sub| (the division by temp = 0.5 or 2 is exact), plus half an ulp
of lg_j - max (below 1e-6 for every entry above e^-16 of the row's largest) and a few 1e-7 of expf, sum and division;
the error of max itself is common to the row and cancels.  Entry j then errs by at most (its own - the p-weighted mean
of the others'), twice the single bound.  For |lg| < 128 that is 2 * 3.8e-6 + ~1.3e-6 < RTOL; from 128 on the ulp
doubles and fp32 - the reference's included - can no longer promise 1e-5 per entry.  So the large rows keep |lg| < 128:
Q to +-80 and log pi to +-40 at temp = 2 (|lg| < 66), Q to +-40 and log pi to +-20 at temp = 0.5 (|lg| < 120, and
above 88.7 in rows where exp() overflows fp32 unless the maximum is subtracted first - asserted below)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_heads_gpu import EINVAL, ENOMEM, K_REF32, LG_COUNT, RTOL, _L, _dev, _exact, _nan, _rc, _untouched
from tests.test_heads_gpu import _check

pytestmark = pytest.mark.gpu

DISCOUNT, REWARD_SCALE, CONS_W, GAP, GRAD_SCALE = 0.95, 10.0, 5.0, 5.0, 0.25
LOG_ALPHA = 0.2
# slots of the metric record this kernel writes (include/tacorl_hip.h TACORL_LG_*)
SLOT = {"bell1": 3, "bell2": 4, "cons1": 5, "cons2": 6, "qloss1": 7, "qloss2": 8, "alpha_p": 9, "alpha_p_loss": 10,
        "q1_data": 11, "q1_rand": 12, "q1_pol": 13, "q2_data": 14, "q2_rand": 15, "q2_pol": 16}

# name: (B, n, A, temp, deterministic_backup, log_alpha_prime or None, large rows: 0 none, (Q, log pi) magnitudes)
CASES = {
    "B1_n1": (1, 1, 7, 0.5, True, -0.3, 0),
    "B1_n42_nolagrange": (1, 42, 16, 2.0, False, None, 0),
    "B5_n4_clamped": (5, 4, 7, 2.0, False, 14.0, 0),
    "B5_n21_nolagrange": (5, 21, 16, 0.5, True, None, 0),
    "B5_n22_clamped": (5, 22, 16, 2.0, True, 14.0, 0),
    "B37_n22_tiny": (37, 22, 7, 0.5, False, -20.0, 0),
    "B37_n21": (37, 21, 7, 2.0, True, -0.3, 0),
    "B37_n32_clamped_large": (37, 32, 16, 2.0, True, 14.0, (80.0, 40.0)),
    "B37_n42_large": (37, 42, 16, 0.5, False, -0.3, (40.0, 20.0)),
    "B1027_n4": (1027, 4, 16, 0.5, False, -0.3, 0),
    "B1027_n32_nolagrange_large": (1027, 32, 7, 2.0, True, None, (80.0, 40.0)),
    "B1027_n1_tiny": (1027, 1, 16, 2.0, False, -20.0, 0),
}


def _inputs(case):
    B, n, A, temp, det, lap, large = CASES[case]
    g = torch.Generator().manual_seed(1000 + list(CASES).index(case))
    R = (3 * n + 1) * B
    x = dict(q=[torch.randn(R, generator=g) * 2 for _ in range(2)], tq=[torch.randn(B, generator=g) * 2 for _ in range(2)],
             lpc=torch.randn(n * B, generator=g) * 3, lpn=torch.randn(n * B, generator=g) * 3,
             nlp=torch.randn(B, generator=g) * 2, reward=(torch.rand(B, generator=g) < 0.3).float(),
             done=(torch.rand(B, generator=g) < 0.3).float(), la=torch.tensor([LOG_ALPHA]),
             lap=None if lap is None else torch.tensor([lap]))
    rows = lambda b: B + torch.arange(3 * n) * B + b  # noqa: E731  the 3n sampled rows of sample b
    if large:  # every second row from 3 on: Q, target Q and the log-probabilities at the large magnitudes
        qm, lm = large
        big = torch.arange(3, B, 2)
        for i in range(2):
            for b in big.tolist():
                r = rows(b)
                x["q"][i][r] = (torch.rand(3 * n, generator=g) * 2 - 1) * qm
                x["q"][i][r[(b + i) % (3 * n)]] = qm if b % 4 == 3 else -qm
            x["q"][i][big] = (torch.rand(len(big), generator=g) * 2 - 1) * qm
            x["tq"][i][big] = (torch.rand(len(big), generator=g) * 2 - 1) * qm
        for b in big.tolist():
            k = torch.arange(n) * B + b
            x["lpc"][k] = (torch.rand(n, generator=g) * 2 - 1) * lm
            x["lpn"][k] = (torch.rand(n, generator=g) * 2 - 1) * lm
            if b % 8 == 3:  # a row whose logits are all far below zero: exp() underflows unless the maximum is subtracted
                for i in range(2):
                    x["q"][i][rows(b)] = -qm + torch.rand(3 * n, generator=g) * 4
                x["lpc"][k] = lm - torch.rand(n, generator=g) * 4
                x["lpn"][k] = lm - torch.rand(n, generator=g) * 4
        # large values on a grid of 1/64: q - log pi of the current / next groups is then exact in fp32 as in fp64 and
        # only the random group (q - log 0.5^A) rounds at |q - sub| >= 32
        for t in x["q"] + x["tq"] + [x["lpc"], x["lpn"]]:
            t.copy_(torch.where(t.abs() > 8, (t * 64).round() / 64, t))
    # (reward, done) = (1, 0) and (0, 1); rows taken modulo B so that every B gets some
    x["reward"][0 % B], x["done"][0 % B] = 1.0, 0.0
    x["reward"][1 % B], x["done"][1 % B] = 0.0, 1.0
    # tie row: all 3n logits equal (to the rounding of log 0.5^A in fp32) - a uniform softmax
    b = 2 % B
    k = torch.arange(n) * B + b
    x["lpc"][k], x["lpn"][k] = -2.5, -2.5
    for i in range(2):
        r = rows(b)
        x["q"][i][r[:n]] = 1.0 + A * math.log(0.5)
        x["q"][i][r[n:]] = 1.0 - 2.5
    return x


def _ref(case, x, dt):
    """cql_offline_lightning.py:284-314 (Bellman target, MSE), 357-398 (CQL log-sum-exp, Lagrange) on the kernel's row
    layout [data B | random nB | current nB | next nB], sample-major k B + b.  Returns the gradients (times grad_scale),
    the logged scalars and the mean |summand| of every scalar."""
    B, n, A, temp, det, lap, _ = CASES[case]
    q = [t.to(dt).requires_grad_() for t in x["q"]]
    tq, lpc, lpn, nlp = [t.to(dt) for t in x["tq"]], x["lpc"].to(dt), x["lpn"].to(dt), x["nlp"].to(dt)
    reward, done = x["reward"].to(dt), x["done"].to(dt)
    alpha = x["la"].to(dt)[0].exp()
    lapt = None if lap is None else x["lap"].to(dt).requires_grad_()
    qn = torch.min(tq[0], tq[1])
    if not det:
        qn = qn - alpha * nlp
    y = REWARD_SCALE * reward + (1.0 - done) * DISCOUNT * qn
    out, scale, lg_max, lg_top, raw, raw_scale = {}, {}, 0.0, -math.inf, [], 0.0
    alpha_p = None if lap is None else lapt[0].exp().clamp(0.0, 1000000.0)
    for i in range(2):
        qd = q[i][:B]
        qr, qc, qx = [q[i][B + gI * n * B: B + (gI + 1) * n * B].view(n, B).t() for gI in range(3)]
        cat = torch.cat([qr - math.log(0.5 ** A), qc - lpc.view(n, B).t(), qx - lpn.view(n, B).t()], 1) / temp
        lg_max, lg_top = max(lg_max, cat.detach().abs().max().item()), max(lg_top, cat.detach().max().item())
        lse = torch.logsumexp(cat, 1)
        cons = lse.mean() * CONS_W * temp - qd.mean() * CONS_W
        s_cons = (lse.detach().abs().mean() * CONS_W * temp + qd.detach().abs().mean() * CONS_W)
        if lap is not None:
            raw.append(cons.detach() - GAP)
            raw_scale = raw_scale + s_cons + GAP
            cons = alpha_p * (cons - GAP)
            s_cons = alpha_p.detach() * (s_cons + GAP)
        bell = F.mse_loss(qd, y)
        loss = bell + cons
        out[f"dq{i + 1}"], = torch.autograd.grad(loss * GRAD_SCALE, q[i], retain_graph=True)
        k = str(i + 1)
        out["bell" + k], scale["bell" + k] = bell.detach(), ((qd - y) ** 2).detach().mean()
        out["cons" + k], scale["cons" + k] = cons.detach(), s_cons
        out["qloss" + k], scale["qloss" + k] = loss.detach(), scale["bell" + k] + s_cons
        out[f"q{k}_data"], scale[f"q{k}_data"] = qd.detach().mean(), qd.detach().abs().mean()
        out[f"q{k}_rand"], scale[f"q{k}_rand"] = qr.detach().mean(), qr.detach().abs().mean()
        out[f"q{k}_pol"], scale[f"q{k}_pol"] = qc.detach().mean(), qc.detach().abs().mean()
        out["cons_t" + k] = cons
    if lap is not None:
        ap_loss = (-out["cons_t1"] - out["cons_t2"]) * 0.5
        g, = torch.autograd.grad(ap_loss * GRAD_SCALE, lapt)
        out["g_lap"], scale["g_lap"] = g[0], 0.5 * raw_scale * lapt.detach()[0].exp() * GRAD_SCALE
        out["alpha_p"], scale["alpha_p"] = alpha_p.detach(), alpha_p.detach()
        out["alpha_p_loss"], scale["alpha_p_loss"] = ap_loss.detach(), 0.5 * (scale["cons1"] + scale["cons2"])
    del out["cons_t1"], out["cons_t2"]
    return out, scale, (lg_max, lg_top)


_REFS = {}


def _refs(case):
    """Inputs and both references of a case, computed once and shared (never modified)."""
    if case not in _REFS:
        x = _inputs(case)
        r64, sc, lg_max = _ref(case, x, torch.float64)
        r32, _, _ = _ref(case, x, torch.float32)
        _REFS[case] = (x, r64, r32, sc, lg_max)
    return _REFS[case]


def _run(case, x, dev):
    from tacorl_amd import ops

    B, n, A, temp, det, lap, _ = CASES[case]
    R = (3 * n + 1) * B
    T = {k: ([t.to(dev) for t in v] if isinstance(v, list) else None if v is None else v.to(dev)) for k, v in x.items()}
    dq = [_nan(R + 8, dev=dev) for _ in range(2)]
    logs, g_lap = _nan(LG_COUNT + 4, dev=dev), _nan(2, dev=dev)
    ws = torch.full((_L().lib().tacorl_cql_ws_bytes(B) // 4,), float("nan"), device=dev)
    ops.call("tacorl_cql_loss", ops.ptr(T["q"][0]), ops.ptr(T["q"][1]), ops.ptr(dq[0]), ops.ptr(dq[1]),
             ops.ptr(T["tq"][0]), ops.ptr(T["tq"][1]), ops.ptr(T["lpc"]), ops.ptr(T["lpn"]), ops.ptr(T["nlp"]),
             ops.ptr(T["reward"]), ops.ptr(T["done"]), ops.ptr(T["la"]), ops.ptr(T["lap"]), B, n, A, DISCOUNT,
             REWARD_SCALE, temp, CONS_W, GAP, int(det), GRAD_SCALE, ops.ptr(g_lap), ops.ptr(logs), ops.ptr(ws),
             ws.numel() * 4, ops.stream())
    torch.cuda.synchronize()
    return [t.cpu() for t in dq], logs.cpu(), g_lap.cpu()


def _check_scalar(name, got, ref, ref32, summand):
    """The rule of _check for one logged scalar: the block's median replaced by the mean |summand| of the scalar."""
    got, ref, ref32, summand = float(got), float(ref), float(ref32), float(summand)
    assert math.isfinite(got), f"{name}: {got}"
    tol = RTOL * (abs(ref) + abs(summand)) + K_REF32 * abs(ref32 - ref)
    worst = abs(got - ref) / max(tol, 1e-300)
    print(f"tolerance-use {name}: {worst:.3g}")
    assert worst <= 1.0, f"{name}: {got} vs {ref}: {worst:.3g} x its tolerance"


@pytest.mark.parametrize("case", list(CASES))
def test_cql_loss_fp64(case):
    dev = _dev()
    B, n, A, temp, det, lap, large = CASES[case]
    x, r64, r32, sc, (lg_max, lg_top) = _refs(case)
    for k, v in r32.items():  # the fp32 reference itself stays finite (checked on the CPU)
        assert torch.isfinite(v).all(), f"fp32 reference {k} is not finite"
    assert lg_max < 128.0, lg_max  # (module docstring)
    if large and temp == 0.5:
        assert lg_top > 88.8, lg_top  # exp() of the largest logit overflows fp32: the maximum must be subtracted
    if B >= 2:
        assert x["reward"][0] == 1 and x["done"][0] == 0 and x["reward"][1] == 0 and x["done"][1] == 1
    dq, logs, g_lap = _run(case, x, dev)
    for i in range(2):
        tag = f"{case} dq{i + 1}"
        _check(f"{tag} data rows", dq[i][:B], r64[f"dq{i + 1}"][:B], r32[f"dq{i + 1}"][:B])
        _check(f"{tag} sampled rows", dq[i][B:(3 * n + 1) * B], r64[f"dq{i + 1}"][B:], r32[f"dq{i + 1}"][B:])
        _untouched(f"{tag} guard", dq[i][(3 * n + 1) * B:])
    written = set()
    for k, slot in SLOT.items():
        if k in r64:
            _check_scalar(f"{case} {k}", logs[slot], r64[k], r32[k], sc[k])
            written.add(slot)
    _untouched(f"{case} log slots of other kernels", logs[[s for s in range(LG_COUNT + 4) if s not in written]])
    if lap is None:
        _untouched(f"{case} g_log_alpha_prime without a Lagrange weight", g_lap)
    else:
        _untouched(f"{case} g_log_alpha_prime guard", g_lap[1:])
        if lap == 14.0:  # e^14 > 1e6: alpha' is the clamp bound and torch.clamp passes no gradient
            assert logs[SLOT["alpha_p"]].item() == 1000000.0 and r64["alpha_p"].item() == 1000000.0
            assert g_lap[0].item() == 0.0 and r64["g_lap"].item() == 0.0
        else:
            assert r64["g_lap"].item() != 0.0
            _check_scalar(f"{case} g_log_alpha_prime", g_lap[0], r64["g_lap"], r32["g_lap"], sc["g_lap"])


def test_cql_loss_run_to_run_identical():
    """Fixed summation order (per-wave partials, folded in index order): two runs of the B = 1027 case agree bitwise."""
    dev = _dev()
    x = _refs("B1027_n4")[0]
    a, b = _run("B1027_n4", x, dev), _run("B1027_n4", x, dev)
    for name, u, v in (("dq1", a[0][0], b[0][0]), ("dq2", a[0][1], b[0][1]), ("logs", a[1], b[1]),
                       ("g_log_alpha_prime", a[2], b[2])):
        # bit patterns: the NaN guards compare equal too
        _exact(f"run-to-run {name}", u.view(torch.int32), v.view(torch.int32))


def test_cql_loss_refuses():
    """n = 43 (3n > 128), n = 0 and a workspace one byte short are refused before anything is launched."""
    from tacorl_amd import ops

    dev = _dev()
    B, A = 5, 7
    buf = torch.zeros((3 * 43 + 1) * B, device=dev)
    dq, logs, g_lap = [_nan((3 * 43 + 1) * B, dev=dev) for _ in range(2)], _nan(LG_COUNT, dev=dev), _nan(1, dev=dev)
    need = _L().lib().tacorl_cql_ws_bytes(B)
    assert need == 2 * 4 * 10 * 4  # two workgroups of four waves, ten partial sums each
    ws = _nan(need // 4, dev=dev)

    def run(n, ws_bytes):
        p = ops.ptr(buf)
        return _rc("tacorl_cql_loss", p, p, ops.ptr(dq[0]), ops.ptr(dq[1]), p, p, p, p, p, p, p, p, p, B, n, A, DISCOUNT,
                   REWARD_SCALE, 0.5, CONS_W, GAP, 1, GRAD_SCALE, ops.ptr(g_lap), ops.ptr(logs), ops.ptr(ws), ws_bytes,
                   ops.stream())

    assert run(43, need) == EINVAL
    assert run(0, need) == EINVAL
    assert run(4, need - 1) == ENOMEM
    torch.cuda.synchronize()
    for name, t in (("dq1", dq[0]), ("dq2", dq[1]), ("logs", logs), ("g_log_alpha_prime", g_lap), ("workspace", ws)):
        _untouched(f"refused call: {name}", t)
    assert run(42, need) == 0  # the widest accepted
    torch.cuda.synchronize()
    assert torch.isfinite(dq[0][:(3 * 42 + 1) * B]).all()
