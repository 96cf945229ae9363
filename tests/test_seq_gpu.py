"""Kernel-level tests of the sequence side: the plan-recognition transformer's kernels (attention, LayerNorm, the glue
between its GEMMs), the action decoder's (input assembly and projection, the logistic-mixture loss, the ReLU-RNN
backward glue), the split-K recurrence GEMM, and PlanRecognition.backward as a whole.

Every output is compared with an fp64 evaluation of the reference's own expressions (oracle/tacorl_oracle.py where it has
them), gradients by torch.autograd on that fp64 graph - never with the kernels' closed forms - at the shapes where the
generic code runs (two cameras: d_model 64; the real-world window T = 32), at the limits the launchers enforce, and at
workgroup and grid-stride boundaries.  Outputs are filled with NaN first; where the ABI has a leading dimension it is
wider than the rows, and the padding and a guard tail behind the written range must stay untouched.

Tolerances, elementwise:  |got - ref64| <= RTOL * (|s| + median|s| of the block) + K_REF32 * |ref32 - ref64|
where ref32 is the same reference evaluated in fp32 (what the reference itself computes) and s is ref64, or, for sums,
the same sum over the magnitudes of its terms (what an fp32 summation's rounding error is proportional to).  Copies,
masks, selections and fp32 expressions of one rounding are compared exactly."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM = -22, -12
F32_EPS = torch.finfo(torch.float32).eps
NAN = float("nan")
# A handful of fp32 roundings per element (6e-8 each), or an fp32 sum measured against the sum of its terms' magnitudes:
# 1e-5 leaves a margin of ~100x over one rounding per term.
RTOL = 1e-5
# Where the reference's own fp32 evaluation loses digits, the kernel may lose as many, within a small multiple.
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


def O_():
    from oracle import tacorl_oracle as O

    return O


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
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bad = (got != ref) & ~(torch.isnan(got) & torch.isnan(ref)) if got.is_floating_point() else got != ref
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.numel()} differ, first at {bad.nonzero()[0].tolist()}: " \
                          f"{got[bad][0].item()} vs {ref[bad][0].item()}"


def _untouched(name, t):
    assert torch.isnan(t.detach().cpu().float()).all(), f"{name}: padding / guard elements were written"


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ============================================================================ attention
def _att_ref(qkv, d_out, B, T, D, H, keep, ks, dt):
    """nn.MultiheadAttention's core as the oracle's plan_recognition writes it: out and d(out . d_out)/d qkv."""
    hd = D // H
    q_ = qkv.to(dt).requires_grad_()
    sh = lambda t: t.reshape(B, T, H, hd).permute(0, 2, 1, 3)  # noqa: E731
    q, k, v = (sh(t) for t in q_.split(D, dim=-1))
    att = torch.softmax((q / math.sqrt(hd)) @ k.transpose(-1, -2), dim=-1)
    if keep is not None:
        att = att * keep.to(dt) * ks
    o = (att @ v).permute(0, 2, 1, 3).reshape(B * T, D)
    g, = torch.autograd.grad((o * d_out.to(dt)).sum(), q_)
    return o.detach(), g


def _att_scales(qkv, d_out, B, T, D, H, keep, ks):
    """Magnitudes of the terms of every sum the attention forward and backward take (fp64): out = sum_j p w v,
    dq / dk = sum ds k / q, dv = sum p w dO, ds = p (w dO.v - sum_j p w dO.v); a probability's relative error from fp32
    logits of magnitude |q|.|k| / sqrt(hd) is that magnitude times eps, expressed here in units of RTOL."""
    hd = D // H
    sh = lambda t: t.reshape(B, T, H, hd).permute(0, 2, 1, 3)  # noqa: E731
    q, k, v = (sh(t) for t in qkv.double().split(D, dim=-1))
    dO = sh(d_out.double())
    p = torch.softmax((q / math.sqrt(hd)) @ k.transpose(-1, -2), dim=-1)
    sa = (q.abs() / math.sqrt(hd)) @ k.abs().transpose(-1, -2)
    p = p * (1 + sa.amax(-1, keepdim=True) * F32_EPS / RTOL)
    w = keep.double() * ks if keep is not None else torch.ones_like(p)
    dpa = dO.abs() @ v.abs().transpose(-1, -2)
    dsa = p * (dpa * w + (p * w * dpa).sum(-1, keepdim=True))
    un = lambda t: t.permute(0, 2, 1, 3).reshape(B * T, D)  # noqa: E731
    out = un((p * w) @ v.abs())
    dq = un(dsa @ k.abs()) / math.sqrt(hd)
    dk = un(dsa.transpose(-1, -2) @ q.abs()) / math.sqrt(hd)
    dv = un((p * w).transpose(-1, -2) @ dO.abs())
    return out, torch.cat([dq, dk, dv], -1)


def _keep_mask(B, H, T, seed):
    keep = torch.rand(B, H, T, T, generator=torch.Generator().manual_seed(seed)) > 0.25
    keep[0, 0, 0] = False  # a fully dropped row: its output and its share of every gradient are 0
    keep[-1, H - 1, T - 1] = True  # a fully kept one
    return keep


# (T, D, H, B): B H is never a multiple of 16 (the t16 backward's last workgroup is part empty) and B H T crosses the
# forward's 128-thread workgroup
ATT_CASES = {
    "t16_fast_path": (16, 32, 8, 5),
    "t16_d64": (16, 64, 8, 5),
    "t32_d32": (32, 32, 8, 5),
    "t32_d64": (32, 64, 8, 3),
    "hd1_t1": (1, 8, 8, 17),
    "hd3_t5": (5, 24, 8, 5),
    "t64_hd16": (64, 128, 8, 3),
}


@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("case", list(ATT_CASES))
def test_attention(case, dropout):
    """tacorl_attention_fwd/_bwd and the dropout entries against fp64 autograd.  T = 16, head_dim 4 with 16-byte aligned
    pointers takes the 16-lanes-per-pair backward; the same call on views 4 bytes off takes the general kernel - both must
    meet the reference.  Batch 1 has logits of magnitude ~30 (one-hot softmax rows)."""
    from tacorl_amd import ops

    dev = _dev()
    T, D, H, B = ATT_CASES[case]
    qkv = _rand(B * T, 3 * D, seed=T * D + B)
    if B > 1:
        qkv.view(B, T, 3 * D)[1, :, :2 * D] *= 4.0  # q.k / sqrt(hd) of std 16
    d_out = _rand(B * T, D, seed=T * D + B + 1)
    keep = _keep_mask(B, H, T, seed=T + D) if dropout else None
    ks = 1.0 / 0.75
    r64 = _att_ref(qkv, d_out, B, T, D, H, keep, ks, torch.float64)
    r32 = _att_ref(qkv, d_out, B, T, D, H, keep, ks, torch.float32)
    s_out, s_dq = _att_scales(qkv, d_out, B, T, D, H, keep, ks)
    kd = keep.to(torch.uint8).to(dev).contiguous() if dropout else None
    for off in ([0, 1] if T == 16 and D // H == 4 else [0]):
        # one allocation per operand, the operand at element `off`: off = 1 moves every pointer off 16-byte alignment
        nq, no = B * T * 3 * D, B * T * D
        qb, db = torch.zeros(nq + off, device=dev), torch.zeros(no + off, device=dev)
        qb[off:] = qkv.flatten().to(dev)
        db[off:] = d_out.flatten().to(dev)
        ob, gb = _nan(no + off + 16, dev=dev), _nan(nq + off + 16, dev=dev)
        P = lambda t: t.data_ptr() + 4 * off  # noqa: E731
        if dropout:
            ops.call("tacorl_attention_dropout_fwd", P(qb), P(ob), ops.ptr(kd), ks, B, T, D, H, ops.stream())
            ops.call("tacorl_attention_dropout_bwd", P(qb), P(db), P(gb), ops.ptr(kd), ks, B, T, D, H, ops.stream())
        else:
            ops.call("tacorl_attention_fwd", P(qb), P(ob), B, T, D, H, ops.stream())
            ops.call("tacorl_attention_bwd", P(qb), P(db), P(gb), B, T, D, H, ops.stream())
        torch.cuda.synchronize()
        tag = f"{case}{'/dropout' if dropout else ''}{'/unaligned' if off else ''}"
        o, g = ob.cpu(), gb.cpu()
        _untouched(f"{tag} out guard", torch.cat([o[:off], o[off + no:]]))
        _untouched(f"{tag} d_qkv guard", torch.cat([g[:off], g[off + nq:]]))
        _check(f"{tag} out", o[off:off + no].view(B * T, D), r64[0], r32[0], scale=s_out)
        _check(f"{tag} d_qkv", g[off:off + nq].view(B * T, 3 * D), r64[1], r32[1], scale=s_dq)
        if dropout:  # the fully dropped row (b 0, head 0, query 0): exactly 0 out
            _exact(f"{tag} dropped row", o[off:off + D // H], torch.zeros(D // H))


def test_attention_refuses_bad_shapes():
    """T > 64, head_dim > 16, D % H != 0 and a NULL keep mask in the dropout entries: EINVAL, nothing written."""
    from tacorl_amd import ops

    dev = _dev()
    n = 65 * 3 * 136
    qkv, dout = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    keep = torch.ones(65 * 65 * 8, dtype=torch.uint8, device=dev)
    out, dq = _nan(n, dev=dev), _nan(n, dev=dev)
    p, s = ops.ptr, ops.stream()
    for T, D, H in ((65, 32, 8), (16, 136, 8), (16, 30, 8)):  # T = 65; head_dim 17; D % H != 0
        assert _rc("tacorl_attention_fwd", p(qkv), p(out), 1, T, D, H, s) == EINVAL, (T, D, H)
        assert _rc("tacorl_attention_bwd", p(qkv), p(dout), p(dq), 1, T, D, H, s) == EINVAL, (T, D, H)
        assert _rc("tacorl_attention_dropout_fwd", p(qkv), p(out), p(keep), 1.25, 1, T, D, H, s) == EINVAL, (T, D, H)
        assert _rc("tacorl_attention_dropout_bwd", p(qkv), p(dout), p(dq), p(keep), 1.25, 1, T, D, H, s) == EINVAL
    assert _rc("tacorl_attention_dropout_fwd", p(qkv), p(out), None, 1.25, 1, 16, 32, 8, s) == EINVAL
    assert _rc("tacorl_attention_dropout_bwd", p(qkv), p(dout), p(dq), None, 1.25, 1, 16, 32, 8, s) == EINVAL
    torch.cuda.synchronize()
    _untouched("out", out)
    _untouched("d_qkv", dq)


# ============================================================================ LayerNorm
def _ln_ref(x, res, w, b, dy, dt):
    """F.layer_norm(x + res) as the oracle's _layer_norm (eps 1e-5), gradients by autograd."""
    x_, w_, b_ = (t.to(dt).requires_grad_() for t in (x, w, b))
    v = x_ + res.to(dt) if res is not None else x_
    y = O_()._layer_norm(v, w_, b_)
    gx, gw, gb = torch.autograd.grad((y * dy.to(dt)).sum(), [x_, w_, b_])
    return y.detach(), gx, gw, gb


def _ln_scales(x, res, w, b, dy):
    """Term magnitudes (fp64): xhat's error from an fp32 mean of |v| is |v| eps, so |xhat| is taken as (|v| + |mean|)
    rstd; dv = rstd (g - mean g - xhat mean(g xhat)), dw = sum_r dy xhat, db = sum_r dy."""
    v = x.double() + (res.double() if res is not None else 0)
    mean = v.mean(-1, keepdim=True)
    rstd = 1 / ((v - mean).pow(2).mean(-1, keepdim=True) + 1e-5).sqrt()
    xs = (v.abs() + mean.abs()) * rstd
    ga = (dy.double() * w.double()).abs()
    y = xs * w.double().abs() + b.double().abs()
    dv = rstd * (ga + ga.mean(-1, keepdim=True) + xs * (ga * xs).mean(-1, keepdim=True))
    return y, dv, (dy.double().abs() * xs).sum(0), dy.double().abs().sum(0)


def _ln_inputs(R, D, seed):
    x, res = _rand(R, D, seed=seed), _rand(R, D, seed=seed + 1, scale=0.5)
    x[0], res[0] = 1.5, 0.0  # a constant row: variance 0 (exact in fp32)
    if R > 2:
        x[2] += 1e3  # rows offset by 1e3
        x[R - 1] += 1e3
    w, b = 1 + _rand(D, seed=seed + 2, scale=0.3), _rand(D, seed=seed + 3, scale=0.3)
    return x, res, w, b, _rand(R, D, seed=seed + 4)


@pytest.mark.parametrize("R", [1, 5, 512, 513, 516, 4097])
@pytest.mark.parametrize("D", [1, 32, 63, 64, 65, 200, 256])
def test_add_layernorm(D, R):
    """tacorl_add_layernorm_fwd/_bwd against fp64 autograd of the oracle's _layer_norm: res given and NULL, stats NULL in
    the forward, accumulate = 0 and accumulate = 1 onto prefilled dw / db.  R = 513..516 is nb = 129 row blocks, the first
    size whose weight-gradient column sum takes two levels.  The column sums are in a fixed order: a second run gives the
    same bits."""
    from tacorl_amd import ops

    dev = _dev()
    x, res, w, b, dy = _ln_inputs(R, D, seed=R + D)
    xd, rd, wd, bd, dyd = (t.to(dev) for t in (x, res, w, b, dy))
    nws = _L().lib().tacorl_add_layernorm_bwd_ws_bytes(R, D)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    pre_w, pre_b = _rand(D, seed=7), _rand(D, seed=8)
    p, s = ops.ptr, ops.stream()
    for with_res in (True, False):
        rr = res if with_res else None
        tag = f"D{D}/R{R}/{'res' if with_res else 'no_res'}"
        y, y2, stats = _nan(R * D + 8, dev=dev), _nan(R * D + 8, dev=dev), _nan(2 * R + 8, dev=dev)
        ops.call("tacorl_add_layernorm_fwd", p(xd), p(rd) if with_res else None, p(wd), p(bd), p(y), p(stats), R, D, 1e-5, s)
        ops.call("tacorl_add_layernorm_fwd", p(xd), p(rd) if with_res else None, p(wd), p(bd), p(y2), None, R, D, 1e-5, s)
        # backward: overwrite (accumulate 0) with res, add onto prefilled dw / db (accumulate 1) without
        acc = 0 if with_res else 1
        dv = _nan(R * D + 8, dev=dev)
        dw = torch.cat([pre_w, torch.full((8,), NAN)]).to(dev) if acc else _nan(D + 8, dev=dev)
        db = torch.cat([pre_b, torch.full((8,), NAN)]).to(dev) if acc else _nan(D + 8, dev=dev)
        ops.call("tacorl_add_layernorm_bwd", p(dyd), p(xd), p(rd) if with_res else None, p(wd), p(stats), p(dv), p(dw), p(db),
                 R, D, acc, p(ws), nws, s)
        dw2, db2 = _nan(D, dev=dev), _nan(D, dev=dev)
        ops.call("tacorl_add_layernorm_bwd", p(dyd), p(xd), p(rd) if with_res else None, p(wd), p(stats), p(dv), p(dw2),
                 p(db2), R, D, 0, p(ws), nws, s)
        torch.cuda.synchronize()
        ref64, ref32 = _ln_ref(x, rr, w, b, dy, torch.float64), _ln_ref(x, rr, w, b, dy, torch.float32)
        sy, sdv, sdw, sdb = _ln_scales(x, rr, w, b, dy)
        for nm, t, n in (("y", y, R * D), ("y (stats NULL)", y2, R * D), ("stats", stats, 2 * R), ("dv", dv, R * D)):
            _untouched(f"{tag} {nm} guard", t[n:])
        _untouched(f"{tag} dw guard", dw[D:])
        _untouched(f"{tag} db guard", db[D:])
        _check(f"{tag} y", y[:R * D].view(R, D), ref64[0], ref32[0], scale=sy)
        _exact(f"{tag} y with stats NULL", y2[:R * D], y[:R * D])
        _check(f"{tag} dv", dv[:R * D].view(R, D), ref64[1], ref32[1], scale=sdv)
        off_w, off_b = (pre_w.double(), pre_b.double()) if acc else (0, 0)
        _check(f"{tag} dw (accumulate {acc})", dw[:D], ref64[2] + off_w, ref32[2] + off_w, scale=sdw + (pre_w.abs() if acc else 0))
        _check(f"{tag} db (accumulate {acc})", db[:D], ref64[3] + off_b, ref32[3] + off_b, scale=sdb + (pre_b.abs() if acc else 0))
        if not acc:  # fixed summation order: the same bits again
            _exact(f"{tag} dw rerun", dw2, dw[:D])
            _exact(f"{tag} db rerun", db2, db[:D])


def test_add_layernorm_refuses():
    """D = 257: EINVAL (forward and backward); a workspace one byte short: ENOMEM; nothing written."""
    from tacorl_amd import ops

    dev = _dev()
    R, D = 40, 257
    buf = torch.zeros(R * D, device=dev)
    y, dv, dw = _nan(R * D, dev=dev), _nan(R * D, dev=dev), _nan(2 * D, dev=dev)
    p, s = ops.ptr, ops.stream()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    assert _rc("tacorl_add_layernorm_fwd", p(buf), None, p(buf), p(buf), p(y), p(dv), R, D, 1e-5, s) == EINVAL
    assert _rc("tacorl_add_layernorm_bwd", p(buf), p(buf), None, p(buf), p(buf), p(dv), p(dw), p(dw), R, D, 0, p(ws),
               ws.numel(), s) == EINVAL
    D = 64
    nws = _L().lib().tacorl_add_layernorm_bwd_ws_bytes(R, D)
    assert _rc("tacorl_add_layernorm_bwd", p(buf), p(buf), None, p(buf), p(buf), p(dv), p(dw), p(dw), R, D, 0, p(ws),
               nws - 1, s) == ENOMEM
    torch.cuda.synchronize()
    for nm, t in (("y", y), ("dv", dv), ("dw", dw)):
        _untouched(nm, t)


# ============================================================================ logistic-mixture loss
def _lm_views(h, B, Tm, Da, K):
    """Kernel heads rows (t B + b) -> the reference's (B, Tm, Da, K) logit_probs, log_scales, means and (B, Tm, 2) grip."""
    n = Da * K
    hv = h.view(Tm, B, -1).transpose(0, 1)
    return (hv[..., 2 * n:3 * n].reshape(B, Tm, Da, K), hv[..., n:2 * n].reshape(B, Tm, Da, K),
            hv[..., :n].reshape(B, Tm, Da, K), hv[..., 3 * n:3 * n + 2])


def _lm_branch(h, act, B, Tm, Da, K, nc, dt):
    """Which of the reference's four torch.where branches each (b, t, a, k) takes, evaluated in dt (and cdf_delta)."""
    lg, ls, mu, _ = _lm_views(h.to(dt), B, Tm, Da, K)
    a = act[:, :Tm, :Da].to(dt).unsqueeze(-1).expand_as(mu)
    inv = torch.exp(-ls.clamp(min=O_().LOG_SIG_MIN))
    hb = 1.0 / (nc - 1)
    delta = torch.sigmoid(inv * (a - mu + hb)) - torch.sigmoid(inv * (a - mu - hb))
    br = torch.where(a < -1.0 + 1e-3, 0, torch.where(a > 1.0 - 1e-3, 1, torch.where(delta > 1e-5, 2, 3)))
    return br, delta


def _lm_case(B, T, Tm, Da, K, nc, seed):
    """Heads [R][ldh] (rows t B + b, ldh > 3 Da K + 2: NaN padding) and actions [B][T][Da + 1], with every branch of the
    loss hit on purpose: x = -1, -0.9995, 0.9995, 1 (the two edge branches), raw log-scales exactly -5 (gradient passes)
    and below (gradient 0), x far from a tiny-scale logistic on either side (log_pdf_mid), and no element within a
    factor e^0.5 of the cdf_delta > 1e-5 threshold, so that fp32 and fp64 take the same branch everywhere."""
    g = torch.Generator().manual_seed(seed)
    R, n = Tm * B, Da * K
    ldh = 3 * n + 2 + 5
    h = torch.full((R, ldh), NAN)
    h[:, :n] = torch.rand(R, n, generator=g) * 1.6 - 0.8
    h[:, n:2 * n] = torch.rand(R, n, generator=g) * 5 - 6.5  # log-scales in [-6.5, -1.5]: a fifth below LOG_SIG_MIN
    h[:, 2 * n:3 * n] = torch.randn(R, n, generator=g) * 2
    h[:, 3 * n:3 * n + 2] = torch.randn(R, 2, generator=g) * 2
    act = torch.rand(B, T, Da + 1, generator=g) * 1.9 - 0.95
    act[..., Da] = torch.randint(-1, 2, (B, T), generator=g).float()  # gripper labels -1 / 0 / 1

    def x_at(r):  # the action the heads row r is scored against, dimension 0
        return act[r % B, r // B, 0]

    for r, v in enumerate((-1.0, -0.9995, 0.9995, 1.0)):
        act[r % B, r // B, 0] = v
    kk = torch.arange(K, dtype=torch.float32)
    for r, lsr in ((4, -5.0), (5, -6.0)):  # clamp bound hit exactly / exceeded; means near x: the cdf_delta branch
        h[r, n:n + K] = lsr
        h[r, :K] = x_at(r) - 0.002 * kk
    for r, side in ((6, 1.0), (7, -1.0)):  # tiny scale, x 0.3 away from every mean: log_pdf_mid
        h[r, n:n + K] = -4.9
        h[r, :K] = x_at(r) + side * (0.3 + 0.01 * kk)
    h[8, 3 * n:3 * n + 2] = 0.5  # tied gripper logits: argmax is class 0, the -1 command
    forced = torch.zeros(R, dtype=torch.bool)
    forced[:9] = True
    for _ in range(3):
        br, delta = _lm_branch(h, act, B, Tm, Da, K, nc, torch.float64)
        near = (br >= 2) & ((delta / 1e-5).log().abs() < 0.5)
        near_rows = near.transpose(0, 1).reshape(R, Da, K)
        if not near_rows.any():
            break
        ls = h[:, n:2 * n].view(R, Da, K)
        ls[near_rows & ~forced.view(R, 1, 1)] = -1.0  # a wide logistic: cdf_delta ~ 0.1
    br64, _ = _lm_branch(h, act, B, Tm, Da, K, nc, torch.float64)
    br32, _ = _lm_branch(h, act, B, Tm, Da, K, nc, torch.float32)
    assert torch.equal(br64, br32), "an element sits at a branch threshold"
    counts = torch.bincount(br64.flatten(), minlength=4)
    assert (counts > 0).all(), counts
    return h, act, ldh


def _lm_scales(h, act, B, Tm, Da, K, nc, gs):
    """Magnitudes (fp64, in the heads' layout) of what the gradient of each mixture component is made of, for the
    tolerance: d mean = -gR w inv (gp + gq) and d log_scale = -gR w (gp plus_in + gq min_in) in the cdf_delta branch, with
    gp = cp (1 - cp) / delta, gq = -cm (1 - cm) / delta - sums whose terms cancel where the bin sits on the logistic's
    centre - and the terms 1 and cp of 1 - cp elsewhere; d logit = -gR (w - p).  cdf_delta = cp - cm itself is known to
    eps (cp + cm) only: log(delta), gp and gq carry the relative error c = (cp + cm) / delta, and the mixture weight w
    that of the log-sum-exp over the components, sum_k w c; both enter at 4 eps."""
    O = O_()
    lg, ls, mu, _ = _lm_views(h.double(), B, Tm, Da, K)
    a = act[:, :Tm, :Da].double().unsqueeze(-1).expand_as(mu)
    lsc = ls.clamp(min=O.LOG_SIG_MIN)
    inv, hb = torch.exp(-lsc), 1.0 / (nc - 1)
    pin, min_in, mid = inv * (a - mu + hb), inv * (a - mu - hb), inv * (a - mu)
    cp, cm = torch.sigmoid(pin), torch.sigmoid(min_in)
    delta = cp - cm
    br, _ = _lm_branch(h, act, B, Tm, Da, K, nc, torch.float64)
    v = torch.where(br == 0, pin - F.softplus(pin), torch.where(br == 1, -F.softplus(min_in), torch.where(
        br == 2, torch.log(delta.clamp(min=1e-300)), mid - lsc - 2 * F.softplus(mid) - math.log((nc - 1) / 2))))
    lp = v + torch.log_softmax(lg, -1)
    w, p = torch.softmax(lp, -1), torch.softmax(lg, -1)
    b2 = br == 2
    c = torch.where(b2, (cp + cm) / delta, torch.ones_like(delta))
    f = 1 + 4 * (c + (w * c).sum(-1, keepdim=True)) * F32_EPS / RTOL
    gp, gq = cp * (1 - cp) / delta, cm * (1 - cm) / delta
    tm = torch.where(b2, inv * (gp + gq), 2 * inv)
    ts = torch.where(b2, gp * pin.abs() + gq * min_in.abs(), 2 * torch.maximum(pin.abs(), min_in.abs()) + 1)
    gR = gs / (B * Tm)
    rows = lambda t: t.transpose(0, 1).reshape(Tm * B, Da * K)  # noqa: E731
    return rows(gR * w * tm * f), rows(gR * w * ts * f), rows(gR * (w * f + p))


def _lm_ref(h, act, B, Tm, Da, K, nc, ga, gs, dt):
    """oracle logistic_mixture_loss (action_decoder_logistic.py:110-235) on the kernel's heads; gradient by autograd."""
    n = Da * K
    h_ = h[:, :3 * n + 2].to(dt).requires_grad_()
    lg, ls, mu, grip = _lm_views(h_, B, Tm, Da, K)
    loss = O_().logistic_mixture_loss(lg, ls, mu, grip, act[:, :Tm].to(dt), num_classes=nc, gripper_alpha=ga)
    g, = torch.autograd.grad(loss * gs, h_)
    return loss.detach(), g


# (B, T, Tm, Da, K, num_classes)
LM_CASES = {
    "K1_Da1": (7, 9, 8, 1, 1, 10),
    "K10_nc256": (9, 12, 11, 6, 10, 256),
    "K16": (5, 16, 15, 6, 16, 10),
    # B Tm Da = 17 280 / 18 000 > 1024 blocks x 16 pairs: the 16-lane kernel's grid-stride loop runs
    "K10_grid_stride": (64, 46, 45, 6, 10, 10),
    "K16_nc256_Da1_grid_stride": (300, 70, 60, 1, 16, 256),
    # 276 480 > 1024 blocks x 256 threads: the scalar kernel's grid-stride loop runs too
    "K10_scalar_grid_stride": (256, 181, 180, 6, 10, 10),
}


@pytest.mark.parametrize("scalar", [0, 1])
@pytest.mark.parametrize("case", list(LM_CASES))
def test_logistic_mixture_loss(case, scalar, monkeypatch):
    """tacorl_logistic_mixture_loss (16-lane kernel, and TACORL_LM_SCALAR=1's one thread per pair) and _finish: the loss
    and d_heads against fp64 autograd of the oracle, the gripper accuracy exactly against the reference's count
    (play_lmp_for_rl.py:166-176: the +-1 command of the argmax class == the label, so a label 0 never counts), the loss's
    bits independent of d_heads and of the lazy finish."""
    from tacorl_amd import ops

    if scalar:
        monkeypatch.setenv("TACORL_LM_SCALAR", "1")
    else:
        monkeypatch.delenv("TACORL_LM_SCALAR", raising=False)
    dev = _dev()
    B, T, Tm, Da, K, nc = LM_CASES[case]
    R, n = Tm * B, Da * K
    ga, gs = 0.5, 3.0
    h, act, ldh = _lm_case(B, T, Tm, Da, K, nc, seed=R + K)
    hd, ad = h.to(dev), act.to(dev)
    nws = _L().lib().tacorl_logistic_mixture_ws_bytes(B, Tm, Da)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    dh = _nan(R, ldh, dev=dev)
    out, out_nograd, out_lazy = _nan(4, dev=dev), _nan(4, dev=dev), _nan(4, dev=dev)
    p, s = ops.ptr, ops.stream()
    args = (B, T, Tm, Da, K, nc, ga, gs)
    ops.call("tacorl_logistic_mixture_loss", p(hd), ldh, p(ad), p(dh), p(out), *args, p(ws), nws, s)
    ops.call("tacorl_logistic_mixture_loss", p(hd), ldh, p(ad), None, p(out_nograd), *args, p(ws), nws, s)
    ops.call("tacorl_logistic_mixture_loss", p(hd), ldh, p(ad), None, None, *args, p(ws), nws, s)
    ops.call("tacorl_logistic_mixture_finish", p(ws), nws, B, Tm, Da, p(out_lazy), s)
    torch.cuda.synchronize()
    o = out.cpu()
    _untouched("out guard", o[2:])
    _exact("loss with d_heads NULL", out_nograd[:2], o[:2])
    _exact("loss by the lazy finish", out_lazy[:2], o[:2])
    l64, g64 = _lm_ref(h, act, B, Tm, Da, K, nc, ga, gs, torch.float64)
    l32, g32 = _lm_ref(h, act, B, Tm, Da, K, nc, ga, gs, torch.float32)
    _check("loss", o[0:1], l64.view(1), l32.view(1))
    grip = h[:, 3 * n:3 * n + 2].view(Tm, B, 2).transpose(0, 1)
    pred = torch.where(grip[..., 1] > grip[..., 0], 1.0, -1.0)
    hits = (pred == act[:, :Tm, Da]).sum()
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    _exact("gripper accuracy", o[1:2], (f32(float(hits)) * (f32(1.0) / f32(float(R)))).view(1))
    d = dh.cpu()
    _untouched("d_heads padding", d[:, 3 * n + 2:])
    below = (h[:, n:2 * n] < -5.0)
    assert below.any() and (h[:, n:2 * n] == -5.0).any()
    _exact("d log_scale below the clamp", d[:, n:2 * n][below], torch.zeros(int(below.sum())))
    assert (g64[:, n:2 * n][h[:, n:2 * n] == -5.0] != 0).all()  # (at the bound the gradient passes)
    s_m, s_s, s_l = _lm_scales(h, act, B, Tm, Da, K, nc, gs)
    _check("d_heads means", d[:, :n], g64[:, :n], g32[:, :n], scale=s_m)
    _check("d_heads log_scales", d[:, n:2 * n][~below], g64[:, n:2 * n][~below], g32[:, n:2 * n][~below], scale=s_s[~below])
    _check("d_heads logit_probs", d[:, 2 * n:3 * n], g64[:, 2 * n:3 * n], g32[:, 2 * n:3 * n], scale=s_l)
    _check("d_heads gripper", d[:, 3 * n:3 * n + 2], g64[:, 3 * n:], g32[:, 3 * n:])


def test_logistic_mixture_loss_refuses():
    """K = 17: EINVAL; a workspace one byte short: ENOMEM (loss and finish); nothing written."""
    from tacorl_amd import ops

    dev = _dev()
    B, T, Tm, Da = 4, 5, 4, 1
    buf = torch.zeros(4096, device=dev)
    out, dh = _nan(4, dev=dev), _nan(4096, dev=dev)
    nws = _L().lib().tacorl_logistic_mixture_ws_bytes(B, Tm, Da)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    p, s = ops.ptr, ops.stream()
    assert _rc("tacorl_logistic_mixture_loss", p(buf), 3 * 17 + 2, p(buf), p(dh), p(out), B, T, Tm, Da, 17, 10, 1.0, 1.0,
               p(ws), nws, s) == EINVAL
    assert _rc("tacorl_logistic_mixture_loss", p(buf), 3 * 10 + 2, p(buf), p(dh), p(out), B, T, Tm, Da, 10, 10, 1.0, 1.0,
               p(ws), nws - 1, s) == ENOMEM
    assert _rc("tacorl_logistic_mixture_finish", p(ws), nws - 1, B, Tm, Da, p(out), s) == ENOMEM
    torch.cuda.synchronize()
    _untouched("loss", out)
    _untouched("d_heads", dh)


# ============================================================================ action-decoder input
def _ad_rows(plan, emb, B, T, Tm, E):
    """x[t B + b] = [plan[b] | emb[b T + t][:E]], t < Tm (action_decoder_logistic.py:279-281, time-major)."""
    e = emb[:, :E].reshape(B, T, E)[:, :Tm].transpose(0, 1)
    return torch.cat([plan.unsqueeze(0).expand(Tm, -1, -1), e], -1).reshape(Tm * B, -1)


def test_build_ad_input():
    """fp32 and bf16 (zero-padded to 128 columns) input rows: exact, ld_emb > E, T > Tm; bf16 EINVAL for P + E > 128,
    E < 1 and an output not 16-byte aligned."""
    from tacorl_amd import ops

    dev = _dev()
    p, s = ops.ptr, ops.stream()
    for B, T, Tm, P, E, ld in ((5, 11, 9, 16, 32, 37), (33, 17, 16, 32, 64, 64), (3, 4, 1, 0, 7, 9), (70, 3, 2, 20, 108, 111)):
        plan, emb = _rand(B, P, seed=B), _rand(B * T, ld, seed=T)
        pd, ed = plan.to(dev), emb.to(dev)
        R = Tm * B
        ref = _ad_rows(plan, emb, B, T, Tm, E)
        out = _nan(R * (P + E) + 9, dev=dev)
        ops.call("tacorl_build_ad_input", p(pd), p(ed), ld, p(out), B, T, Tm, P, E, s)
        ob = torch.full((R * 128 + 72,), NAN, dtype=torch.bfloat16, device=dev)
        ops.call("tacorl_build_ad_input_bf16", p(pd), p(ed), ld, p(ob), B, T, Tm, P, E, s)
        torch.cuda.synchronize()
        o = out.cpu()
        _exact(f"B{B} fp32 rows", o[:R * (P + E)].view(R, P + E), ref)
        _untouched("fp32 guard", o[R * (P + E):])
        b = ob.cpu()
        _exact(f"B{B} bf16 rows", b[:R * 128].view(R, 128)[:, :P + E], ref.to(torch.bfloat16))
        _exact(f"B{B} bf16 zero columns", b[:R * 128].view(R, 128)[:, P + E:], torch.zeros(R, 128 - P - E))
        _untouched("bf16 guard", b[R * 128:])
    buf = torch.zeros(4096, device=dev)
    ob = torch.full((4096,), NAN, dtype=torch.bfloat16, device=dev)
    assert _rc("tacorl_build_ad_input_bf16", p(buf), p(buf), 128, p(ob), 2, 3, 2, 16, 113, s) == EINVAL  # P + E = 129
    assert _rc("tacorl_build_ad_input_bf16", p(buf), p(buf), 128, p(ob), 2, 3, 2, 16, 0, s) == EINVAL  # E = 0
    assert _rc("tacorl_build_ad_input_bf16", p(buf), p(buf), 128, ob[1:].data_ptr(), 2, 3, 2, 16, 32, s) == EINVAL
    torch.cuda.synchronize()
    _untouched("bf16 out after EINVAL", ob)


AD_P = {32: 12, 40: 16, 48: 16, 56: 20, 64: 32}  # K = P + E -> P


@pytest.mark.parametrize("R", [45, 64, 2368])
@pytest.mark.parametrize("H", [16, 48, 512, 528, 2048])
@pytest.mark.parametrize("K", [32, 40, 48, 56, 64])
def test_ad_input_proj(K, H, R):
    """The bf16 MFMA input projection against fp64 on bf16-rounded operands: K = 40 / 56 leave part of the second k-step
    empty, H = 528 is a second blockIdx.y column group of one tile, R not a multiple of the 64-row workgroup."""
    from tacorl_amd import ops

    dev = _dev()
    B, Tm = {45: (5, 9), 64: (8, 8), 2368: (64, 37)}[R]
    T, P = Tm + 2, AD_P[K]
    E, ld = K - P, K - P + 3
    plan, emb = _rand(B, P, seed=K), _rand(B * T, ld, seed=H)
    W, bias = _rand(H, K, seed=R, scale=0.2), _rand(H, seed=R + 1)
    pd, ed, bd = (t.to(dev) for t in (plan, emb, bias))
    # W with a NaN guard behind it: a k-step reading columns >= K of the last row would turn its outputs into NaN
    wd = torch.cat([W.flatten(), torch.full((64,), NAN)]).to(dev)
    out = _nan(R * H + 64, dev=dev)
    ops.call("tacorl_ad_input_proj", ops.ptr(pd), ops.ptr(ed), ld, ops.ptr(wd), ops.ptr(bd), ops.ptr(out), B, T, Tm, P, E, H,
             ops.stream())
    torch.cuda.synchronize()
    o = out.cpu()
    _untouched("out guard", o[R * H:])
    x = _ad_rows(plan, emb, B, T, Tm, E).to(torch.bfloat16).double()
    w = W.to(torch.bfloat16).double()
    ref = x @ w.t() + bias.double()
    _check(f"K{K} H{H} R{R}", o[:R * H].view(R, H), ref, scale=x.abs() @ w.abs().t() + bias.double().abs())


def test_ad_input_proj_refuses():
    """K = P + E of 24 (< 32), 44 (not a multiple of 8), 72 (> 64); H = 40 (not a multiple of 16); W, b or out not 16-byte
    aligned: EINVAL, nothing written."""
    from tacorl_amd import ops

    dev = _dev()
    buf = torch.zeros(1 << 16, device=dev)
    out = _nan(1 << 16, dev=dev)
    p, s = ops.ptr, ops.stream()
    q = buf[1:].data_ptr()

    def run(P, E, H, w=None, b=None, o=None):
        return _rc("tacorl_ad_input_proj", p(buf), p(buf), 80, w or p(buf), b or p(buf), o or p(out), 4, 5, 4, P, E, H, s)

    for P, E, H in ((8, 16, 64), (12, 32, 64), (32, 40, 64), (16, 32, 40)):
        assert run(P, E, H) == EINVAL, (P, E, H)
    assert run(16, 32, 64, w=q) == EINVAL
    assert run(16, 32, 64, b=q) == EINVAL
    assert run(16, 32, 64, o=out[1:].data_ptr()) == EINVAL
    torch.cuda.synchronize()
    _untouched("out", out)


@pytest.mark.parametrize("accumulate", [0, 1, 2])
def test_ad_input_bwd(accumulate):
    """d_plan[b] = sum_{t < Tm} dx[t B + b][:P]; d_emb rows t < Tm get dx[.][P:] (overwritten, added, overwritten); rows
    t >= Tm are untouched (0, 1) or zeroed (2); columns E..ld_emb are never written."""
    from tacorl_amd import ops

    dev = _dev()
    B, T, Tm, P, E, ld = 37, 9, 7, 16, 32, 35
    dx = _rand(Tm * B, P + E, seed=1)
    pre = _rand(B * T, ld, seed=2)
    d_emb = pre.to(dev)
    d_plan = _nan(B * P + 8, dev=dev)
    dxd = dx.to(dev)  # (device copies are held in names until the launch has run: a freed temporary's block is reused)
    ops.call("tacorl_ad_input_bwd", ops.ptr(dxd), ops.ptr(d_plan), ops.ptr(d_emb), ld, B, T, Tm, P, E, accumulate,
             ops.stream())
    torch.cuda.synchronize()
    x = dx.view(Tm, B, P + E)
    dp = d_plan.cpu()
    _untouched("d_plan guard", dp[B * P:])
    _check("d_plan", dp[:B * P].view(B, P), x[..., :P].double().sum(0), scale=x[..., :P].double().abs().sum(0))
    ref = pre.clone().view(B, T, ld)
    v = x[..., P:].transpose(0, 1)
    ref[:, :Tm, :E] = pre.view(B, T, ld)[:, :Tm, :E] + v if accumulate == 1 else v
    if accumulate == 2:
        ref[:, Tm:, :E] = 0
    _exact("d_emb", d_emb.cpu(), ref.view(B * T, ld))


@pytest.mark.parametrize("n", [1000, 2048 * 256 + 5])
def test_relu_mask_mul(n):
    """out = (dy (+ add)) [h > 0]: h exactly +-0 gives 0; n = 2048 x 256 + 5 runs the grid-stride loop."""
    from tacorl_amd import ops

    dev = _dev()
    dy, add, h = _rand(n, seed=1), _rand(n, seed=2), _rand(n, seed=3)
    h[::7] = 0.0
    h[3::11] = -0.0
    h[5::13] = 1.5e-38  # (the smallest normal magnitude: still > 0)
    dyd, addd, hd = dy.to(dev), add.to(dev), h.to(dev)
    for with_add in (False, True):
        out = _nan(n + 8, dev=dev)
        ops.call("tacorl_relu_mask_mul", ops.ptr(dyd), ops.ptr(addd) if with_add else None, ops.ptr(hd),
                 ops.ptr(out), n, ops.stream())
        torch.cuda.synchronize()
        o = out.cpu()
        _untouched("guard", o[n:])
        ref = torch.where(h > 0, dy + add if with_add else dy, torch.zeros(()))
        _exact(f"relu_mask_mul add={with_add}", o[:n], ref)


# ============================================================================ transformer glue
@pytest.mark.parametrize("R,T,D,Dp,ldx", [(37 * 16, 16, 30, 32, 36), (5 * 32, 32, 64, 64, 64), (3, 1, 1, 8, 5),
                                          (7 * 32, 32, 61, 64, 70)])
def test_add_rows_bcast(R, T, D, Dp, ldx):
    """out[r] = [x[r][:D] | 0 ... Dp] + add[r % T]: exact, ldx > D, zero columns D..Dp."""
    from tacorl_amd import ops

    dev = _dev()
    x, add = _rand(R, ldx, seed=R), _rand(T, Dp, seed=T)
    out = _nan(R * Dp + 8, dev=dev)
    xd, addd = x.to(dev), add.to(dev)
    ops.call("tacorl_add_rows_bcast", ops.ptr(xd), ldx, ops.ptr(addd), ops.ptr(out), R, T, D, Dp, ops.stream())
    torch.cuda.synchronize()
    o = out.cpu()
    _untouched("guard", o[R * Dp:])
    xp = torch.cat([x[:, :D], torch.zeros(R, Dp - D)], 1)
    _exact("add_rows_bcast", o[:R * Dp].view(R, Dp), xp + add.repeat(R // T + 1, 1)[:R])


@pytest.mark.parametrize("B,T,D", [(37, 16, 32), (3, 32, 64), (300, 1, 7), (5, 33, 65)])
def test_mean_and_bcast_over_t(B, T, D):
    """mean_over_t against fp64; bcast_over_t (the mean's backward) with a scale, overwriting and accumulating: exact."""
    from tacorl_amd import ops

    dev = _dev()
    x = _rand(B * T, D, seed=B)
    out = _nan(B * D + 8, dev=dev)
    src, pre = _rand(B, D, seed=T), _rand(B * T, D, seed=D)
    xd, srcd = x.to(dev), src.to(dev)
    ops.call("tacorl_mean_over_t", ops.ptr(xd), ops.ptr(out), B, T, D, ops.stream())
    sc = 1.0 / T
    dst0, dst1 = _nan(B * T * D + 8, dev=dev), torch.cat([pre.flatten(), torch.full((8,), NAN)]).to(dev)
    ops.call("tacorl_bcast_over_t", ops.ptr(srcd), ops.ptr(dst0), B, T, D, sc, 0, ops.stream())
    ops.call("tacorl_bcast_over_t", ops.ptr(srcd), ops.ptr(dst1), B, T, D, sc, 1, ops.stream())
    torch.cuda.synchronize()
    o = out.cpu()
    _untouched("mean guard", o[B * D:])
    xv = x.view(B, T, D).double()
    _check("mean_over_t", o[:B * D].view(B, D), xv.mean(1), scale=xv.abs().mean(1))
    v = (src * torch.tensor(sc, dtype=torch.float32)).unsqueeze(1).expand(B, T, D).reshape(B * T, D)
    for nm, d, ref in (("bcast_over_t", dst0, v), ("bcast_over_t accumulate", dst1, pre + v)):
        dc = d.cpu()
        _untouched(f"{nm} guard", dc[B * T * D:])
        _exact(nm, dc[:B * T * D].view(B * T, D), ref)


@pytest.mark.parametrize("n", [77, 4096 * 256 + 3])
def test_dropout_mul(n):
    """x = keep ? x / (1 - p) : 0 in place: exact; n = 4096 x 256 + 3 runs the grid-stride loop."""
    from tacorl_amd import ops

    dev = _dev()
    x = _rand(n, seed=n)
    keep = (torch.rand(n, generator=torch.Generator().manual_seed(1)) > 0.1).to(torch.uint8)
    ks = 1.0 / 0.9
    xd = torch.cat([x, torch.full((8,), NAN)]).to(dev)
    kd = keep.to(dev)
    ops.call("tacorl_dropout_mul", ops.ptr(xd), ops.ptr(kd), ks, n, ops.stream())
    torch.cuda.synchronize()
    o = xd.cpu()
    _untouched("guard", o[n:])
    _exact("dropout_mul", o[:n], torch.where(keep.bool(), x * torch.tensor(ks, dtype=torch.float32), torch.zeros(())))


# ============================================================================ split-K recurrence GEMM
# (M per problem, K, N, act, ld_add): N = 30 / 2048 with K >= 512 and few row tiles take the split-K path (the chip is not
# filled), K = 100 the single pass
LIN_CASES = {
    "p1_M3_K512_N30_relu": ([3], 512, 30, 1, 33),
    "p2_M3_256_K2048_N30": ([3, 256], 2048, 30, 0, 32),
    "p2_M3_256_K2048_N2048_relu": ([3, 256], 2048, 2048, 1, 2052),
    "p3_M5_3_256_K100_N2048": ([5, 3, 256], 100, 2048, 0, 2049),
    "p1_M256_K512_N2048": ([256], 512, 2048, 1, 2050),
    "p3_M3_17_3_K2048_N30_relu": ([3, 17, 3], 2048, 30, 1, 31),
}


@pytest.mark.parametrize("case", list(LIN_CASES))
def test_linear_add_fwd(case):
    """y = act(x W^T + b + addend) against fp64, with the workspace NULL, one float short (both: the single pass) and
    exactly tacorl_linear_add_fwd_ws_bytes (the split-K pass + bias_act_reduce); ldx, ldy and ld_add wider than K / N."""
    from tacorl_amd import ops

    dev = _dev()
    Ms, K, N, act, ld_add = LIN_CASES[case]
    npb, ldx, ldy = len(Ms), K + 4, N + 2
    xs = [_rand(M, ldx, seed=10 + i) for i, M in enumerate(Ms)]
    ws_ = [_rand(N, K, seed=20 + i, scale=1 / math.sqrt(K)) for i in range(npb)]
    bs = [_rand(N, seed=30 + i) for i in range(npb)]
    adds = [_rand(M, ld_add, seed=40 + i) for i, M in enumerate(Ms)]
    D = lambda ts: [t.to(dev) for t in ts]  # noqa: E731
    xd, wd, bd, ad = D(xs), D(ws_), D(bs), D(adds)
    need = _L().lib().tacorl_linear_add_fwd_ws_bytes(npb, ops.int_array(Ms), K, N)
    modes = [("ws NULL", None, 0)] + ([("ws one float short", need - 4, need - 4), ("ws exact", need, need)] if need else [])
    refs = []
    for i, M in enumerate(Ms):
        x, w = xs[i][:, :K].double(), ws_[i].double()
        z = x @ w.t() + bs[i].double() + adds[i][:, :N].double()
        refs.append((F.relu(z) if act else z, x.abs() @ w.abs().t() + bs[i].double().abs() + adds[i][:, :N].double().abs()))
    for tag, alloc, nb in modes:
        ys = [_nan(M * ldy + 8, dev=dev) for M in Ms]
        wsb = torch.empty(max(alloc or 0, 1), dtype=torch.uint8, device=dev)
        ops.call("tacorl_linear_add_fwd", npb, ops.ptr_array(xd), ldx, ops.ptr_array(wd), ops.ptr_array(bd), ops.ptr_array(ad),
                 ld_add, ops.ptr_array(ys), ldy, ops.int_array(Ms), K, N, act, 0, ops.ptr(wsb) if alloc else None, nb,
                 ops.stream())
        torch.cuda.synchronize()
        for i, M in enumerate(Ms):
            y = ys[i].cpu()
            _untouched(f"{tag} y guard", y[M * ldy:])
            y = y[:M * ldy].view(M, ldy)
            _untouched(f"{tag} y padding", y[:, N:])
            _check(f"{case} {tag} problem {i}", y[:, :N], refs[i][0], scale=refs[i][1])


# ============================================================================ PlanRecognition.backward
def _pr_module(D, T, A, dropout_p, seed):
    from tacorl_amd.networks.plan_recognition import PlanRecognition

    pr = PlanRecognition(state_dim=D, latent_plan_dim=A, device=_dev(), num_heads=8, num_layers=2, encoder_hidden_size=2048,
                         fc_hidden_size=4096, max_position_embeddings=T, dropout_p=dropout_p)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in pr.blk.views.items():
            if k.endswith("weight") and v.dim() == 2:
                v.copy_((torch.rand(v.shape, generator=g) * 2 - 1) / math.sqrt(v.shape[1]))
            elif "norm" in k and k.endswith("weight"):
                v.copy_(1 + 0.1 * torch.randn(v.shape, generator=g))
            else:
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
    return pr


def _pr_masks(B, T, D, FF, H, p, seed):
    """The reference's 1 + 4 L keep masks in its draw order and layouts (oracle plan_recognition's docstring)."""
    g = torch.Generator().manual_seed(seed)
    m = lambda *s: torch.rand(*s, generator=g) >= p  # noqa: E731
    masks = [m(T, B, D)]
    for _ in range(2):
        masks += [m(B, H, T, T), m(T, B, D), m(T, B, FF), m(T, B, D)]
    return masks


class _ReluFollows:
    """F for the oracle inside `with`: its FFN ReLUs (one per layer, in order) take the kernel's decision - ff1 > 0 of the
    module's saved FFN activation - where |z| is below 1e-4 of the layer's mean |z|, a tie the fp32 GEMM may round to
    either side (1.2 M pre-activations per layer at B = 37: a few sit within fp32 rounding of 0), and z > 0 elsewhere."""

    def __init__(self, ff1, keep):
        self.ff1, self.keep, self.l, self.ties = ff1, keep, 0, 0

    def __getattr__(self, name):
        return getattr(F, name)

    def relu(self, z):
        kern = self.ff1[self.l].view(z.shape) > 0
        if self.keep is not None:  # (a dropped unit's kernel value is 0 whatever its sign: not a decision)
            kern = kern | ~self.keep[self.l].permute(1, 0, 2).reshape(z.shape) & (z.detach() > 0)
        tie = z.detach().abs() < 1e-4 * z.detach().abs().mean()
        assert not (kern != (z.detach() > 0))[~tie].any(), "the kernel's ReLU differs away from a tie"
        self.ties += int(tie.sum())
        self.l += 1
        return z * torch.where(tie, kern, z.detach() > 0).to(z.dtype)

    def __enter__(self):
        self.prev, O_().F = O_().F, self
        return self

    def __exit__(self, *exc):
        O_().F = self.prev
        return False


def _pr_ref(P, emb, d_head, A, min_std, dropout, dt, relu=None):
    """The oracle's plan_recognition in dt; the head [mean | var_raw] and the gradients of sum(head * d_head) with respect
    to the embeddings and every parameter (d var_raw chained through the oracle's softplus: d std = d var_raw / sigmoid).
    relu: (ff1, FFN keep masks) of the kernel's forward, for _ReluFollows."""
    Pd = {k: v.to(dt).requires_grad_() for k, v in P.items()}
    e = emb.to(dt).requires_grad_()
    if relu is not None:
        with _ReluFollows(*relu):
            mean, std = O_().plan_recognition(Pd, "", e, min_std=min_std, dropout=dropout)
    else:
        mean, std = O_().plan_recognition(Pd, "", e, min_std=min_std, dropout=dropout)
    vr = torch.log(torch.expm1(std.detach() - min_std))
    dh = d_head.to(dt)
    loss = (mean * dh[:, :A]).sum() + (std * (dh[:, A:] / torch.sigmoid(vr))).sum()
    names = [k for k in Pd if not k.startswith("layernorm.")]
    grads = torch.autograd.grad(loss, [e] + [Pd[k] for k in names], allow_unused=True)
    return torch.cat([mean.detach(), vr], 1), grads[0], dict(zip(names, grads[1:])), std.detach()


def _pr_run(pr, emb, d_head, B, T, compute, masks=None):
    if masks is not None:
        pr.stage_dropout(B, T, masks)
    head = pr.forward(emb, pr.D, B, T, compute, train=True).clone()
    pr.blk.grad.zero_()
    for k, v in pr.blk.grad_views.items():  # every gradient must be written
        if not k.startswith("layernorm."):
            v.fill_(NAN)
    ff1 = [t.cpu() for t in pr.ff1]
    dx = pr.backward(d_head, B, T, compute).clone()
    torch.cuda.synchronize()
    return head.cpu(), dx.cpu(), {k: v.detach().cpu().clone() for k, v in pr.blk.grad_views.items()}, ff1


# (module level: dozens of dependent fp32 GEMMs with K up to 4096, LayerNorms, softmaxes: the magnitude rule of the
# kernel tests with a tolerance ten times wider)
RTOL_MODULE = 1e-4


@pytest.mark.parametrize("dropout_p", [0.0, 0.1])
@pytest.mark.parametrize("D,T", [(32, 16), (64, 16), (32, 32), (64, 32)])
def test_plan_recognition_backward_f32(D, T, dropout_p):
    """PlanRecognition forward + backward on the f32 per-op path (train mode, dropout masks injected in the reference's
    layouts) against fp64 autograd of the oracle's plan_recognition: the head, d emb and every parameter gradient by name.
    d_model 64 / window 32 run the general attention backward and the D = 64 LayerNorms."""
    dev = _dev()
    B, A = 37, (16 if D == 32 else 32)
    pr = _pr_module(D, T, A, dropout_p, seed=D + T)
    emb = _rand(B * T, D, seed=3)
    d_head = _rand(B, 2 * A, seed=4)
    masks = _pr_masks(B, T, D, pr.FF, pr.H, dropout_p, seed=5) if dropout_p else None
    head, dx, grads, ff1 = _pr_run(pr, emb.to(dev), d_head.to(dev), B, T, 0, masks)
    P = {k: v.detach().cpu().clone() for k, v in pr.blk.views.items()}
    drop = (dropout_p, masks) if dropout_p else None
    relu = (ff1, [masks[3], masks[7]] if dropout_p else None)
    h64, dx64, g64, _ = _pr_ref(P, emb.view(B, T, D), d_head, A, pr.min_std, drop, torch.float64, relu)
    h32, dx32, g32, _ = _pr_ref(P, emb.view(B, T, D), d_head, A, pr.min_std, drop, torch.float32, relu)
    tag = f"D{D}/T{T}/p{dropout_p}"
    _check(f"{tag} head", head, h64, h32, rtol=RTOL_MODULE)
    _check(f"{tag} dx", dx, dx64.reshape(B * T, D), dx32.reshape(B * T, D), rtol=RTOL_MODULE)
    for k, g in g64.items():
        _check(f"{tag} d {k}", grads[k], g, g32[k], rtol=RTOL_MODULE)


def _relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# Bounds on the relative error (norm) against the oracle with bf16 operand rounding: three times the worst measured on an
# MI355X - head 6.7e-4 (both paths), d emb 6.8e-4 (fused; per-op 1.2e-4), parameter gradients 3.4e-3 (mean_fc.weight,
# both paths; the encoder layers' at most 1.8e-3, fused linear1.weight of layer 1).
BF16_BOUND = {"head": 2e-3, "dx": 2e-3, "grad": 1e-2}


def test_plan_recognition_backward_bf16():
    """The bf16 per-op backward and the fused one-launch backward (d_model 32, window 16) against the oracle with the
    MFMA's operand rounding (operand_rounding(bf16)): the head, d emb and every parameter gradient by name."""
    dev = _dev()
    B, T, D, A = 37, 16, 32, 16
    pr = _pr_module(D, T, A, 0.0, seed=77)
    emb, d_head = _rand(B * T, D, seed=6), _rand(B, 2 * A, seed=7)
    P = {k: v.detach().cpu().clone() for k, v in pr.blk.views.items()}
    with O_().operand_rounding(torch.bfloat16):
        h_r, dx_r, g_r, std_r = _pr_ref(P, emb.view(B, T, D), d_head, A, pr.min_std, None, torch.float32)
    for fused in (False, True):
        pr.fused_train = pr.fused_backward = fused
        head, dx, grads, _ = _pr_run(pr, emb.to(dev), d_head.to(dev), B, T, 1)
        if fused:
            assert pr._fused_saved == (B, T), "the one-launch backward was not taken"
        tag = "fused" if fused else "per-op"
        # (the head as [mean | std]: var_raw recovered from an fp32 std loses digits where softplus is flat)
        std = F.softplus(head[:, A:].double()) + pr.min_std
        errs = {"head": _relerr(torch.cat([head[:, :A].double(), std], 1), torch.cat([h_r[:, :A], std_r], 1)),
                "dx": _relerr(dx, dx_r.reshape(B * T, D))}
        errs.update({f"d {k}": _relerr(grads[k], g) for k, g in g_r.items()})
        for k, e in errs.items():
            bound = BF16_BOUND.get(k, BF16_BOUND["grad"])
            print(f"tolerance-use bf16 {tag} {k}: {e / bound:.3g} (relerr {e:.3g})")
            assert e <= bound, (tag, k, e, bound)
