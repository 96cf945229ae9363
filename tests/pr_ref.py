"""fp64 restatement of the one-launch plan-recognition forward (tacorl_amd/csrc/pr_fused.hip: pr_encoder_fused_kernel<1|2>,
pr_encoder_fused64_kernel<1|2>, pr_head_compose_kernel), stage by stage, with the rounding points of the kernels, seeded
problems that make its checks discriminating, and the a-priori bounds tests/test_pr_fp64_gpu.py holds the kernels to
(tests/test_pr_ref_cpu.py shows what those bounds still detect).  Plain torch on the CPU: no GPU, no kernel of this
repository, not built on oracle/tacorl_oracle.py - the oracle is one of the things compared against this file.

Rounding points, read from the kernels (d_model 32 | d_model 64; every bf16 rounding is round-to-nearest-even, `(__bf16)x`):
  x = emb[:, :D] + pos[t]   one fp32 add                                                      (pr_fused.hip:178 | :539)
  MFMA B operands           x, the attention output, x1 (LayerNorm-1 output) and the post-ReLU hidden state are rounded to
                            bf16 when staged into the LDS                          (:186, :298, :366 | :547, :629, :702)
  weight matrices           the bf16 mirror Pb of the parameter block: RNE of the fp32 block (:206, :211, :224, :355 |
                            :568, :595, :641, :650)
  biases                    fp32, the MFMA accumulator's initial value (:261, :314, :363 | :583, :668, :699); b2 starts wave
                            0's accumulator only (:347 | :693)
  logits                    q scaled in fp32 by log2(e) / sqrt(hd) (:278 | :608), then ((q0 k0 + q1 k1) + q2 k2) + q3 k3 in
                            fp32 (:283 | two such chains of 4 added, :614)
  softmax                   2^(s - max) by the hardware exp2, the sum in key order, the hardware reciprocal (:288-289 |
                            :619-620), p v accumulated in key order (:294-296 | :625-626)
  LayerNorm                 v = x + sublayer in fp32 (:317, :407 | :671, :743); mean = sum / D with the sum as a chain of
                            D / 4 values in a lane and two cross-lane adds, centred variance / D the same way,
                            1 / sqrtf(var + 1e-5f), ((v - mean) rstd) w + b, all fp32 (:95-117 | :488-509)
  FFN2                      per-wave fp32 MFMA accumulation over that wave's chunks (wave w: chunks w, w + 4, ... of 256 |
                            128 hidden units), then ((p0 + p1) + p2) + p3 (:403-405 | :740-742)
  pooled                    sum over row tiles, then over lanes, then x (1 / T) (:418-428 | :755-765)
  head / plan               head = bc + sum_d Wc pooled: fp32 scalar chain over D from the fp32 (Wc, bc) of
                            pr_head_compose_kernel (fp32 sums over FC, :1099-1113); sd = (vr > 20 ? vr : log1pf(expf(vr))) +
                            min_std; plan = tanhf(mean + eps sd) (:437-447 | :773-784)
`rounded=False`: no bf16 rounding anywhere.

The hardware exp2 (v_exp_f32) and reciprocal (v_rcp_f32) are taken at 1 ulp, as the VOP1 descriptions of the "AMD Instinct
CDNA3 / CDNA4 Instruction Set Architecture" reference guides give them ("1 ULP accuracy"); 1 ulp <= 2 U32 relative."""
import math

import torch
import torch.nn.functional as F

from tests.mlp_ref import (ACT_FACTOR, C_SUM, E2E_FACTOR, FAULT_RATIO, U32, bf16, bound_use, per_row_relerr,  # noqa: F401
                           relerr)

H = 8                  # heads (PR_H)
MAXL = 4               # PR_MAXL
LN_EPS = 1e-5
POP = 256              # sequences of the population that calibrates the end-to-end rule (E2)
LOUD, QUIET = 1, 2     # sequence 1: logits of magnitude ~ 30 in layer 0; sequence 2: emb x 0.25 (small LayerNorm variance)
LOUD_LOGIT = 30.0
VAR_BIAS = 25.0        # variance_fc biases +25 (first) and -25 (last): both softplus branches and the flat region
LKEYS = ("in_w", "in_b", "out_w", "out_b", "w1", "b1", "w2", "b2", "n1w", "n1b", "n2w", "n2b")  # PrLayerOff order


def chunk(D):
    """Hidden units per FFN chunk: PR_CH = 256, CH6 = 128."""
    return 256 if D == 32 else 128


def _r(t, rounded):
    return bf16(t) if rounded else t


# ------------------------------------------------------------------------------------------------------ stages
# Every stage works on (B, T, .) tensors of one dtype and returns (result, mag): mag = the sum of the magnitudes of the terms
# of every element's sum, sum |x~||w~| + |b|, the scale of its bound (None where the bound is not of that form).
def stage_input(emb, pos):
    T = emb.shape[1]
    return emb + pos[:T], emb.abs() + pos[:T].abs()


def stage_linear(x, W, b, rounded=True):
    """y = x~ W~^T + b (in-projection, out-projection, FFN2); x~, W~: bf16 RNE of x, W."""
    xr, Wr = _r(x, rounded), _r(W, rounded)
    return F.linear(xr, Wr, b), F.linear(xr.abs(), Wr.abs(), b.abs())


def stage_ffn1(x1, W1, b1, rounded=True):
    y, mag = stage_linear(x1, W1, b1, rounded)
    return F.relu(y), mag


def stage_ffn2(h, W2, b2, rounded=True):
    return stage_linear(h, W2, b2, rounded)


def stage_ffn2_kernel_order(h, W2, b2, rounded=True):
    """The same sum in the kernel's order: chunks dealt to four partial sums (wave w: chunks w, w + 4, ...; b2 in wave 0's),
    then ((p0 + p1) + p2) + p3.  A different, valid fp32 evaluation of stage_ffn2."""
    hr, Wr = _r(h, rounded), _r(W2, rounded)
    CH = chunk(W2.shape[0])
    part = []
    for w in range(4):
        p = b2.expand(*h.shape[:-1], -1).clone() if w == 0 else torch.zeros(*h.shape[:-1], W2.shape[0], dtype=h.dtype)
        for c in range(w, W2.shape[1] // CH, 4):
            p = p + hr[..., CH * c: CH * (c + 1)] @ Wr[:, CH * c: CH * (c + 1)].t()
        part.append(p)
    return ((part[0] + part[1]) + part[2]) + part[3], F.linear(hr.abs(), Wr.abs(), b2.abs())


def _heads(t, hd):
    B, T, D = t.shape
    return t.reshape(B, T, D // hd, hd).permute(0, 2, 1, 3)


def stage_attention(qkv, hd_scale=None):
    """softmax(q k^T / sqrt(hd)) v per head on the fp32 q|k|v (no operand rounding).  -> (att (B, T, D), info): info =
    {p (B, H, T, T), sa: max over keys of sum_e |q_e k_e| / sqrt(hd) per (b, h, query), pv: sum_t p |v|}."""
    D = qkv.shape[-1] // 3
    hd = D // H
    q, k, v = (_heads(t, hd) for t in qkv.split(D, dim=-1))
    sc = math.sqrt(hd_scale or hd)
    p = torch.softmax((q / sc) @ k.transpose(-1, -2), dim=-1)
    un = lambda t: t.permute(0, 2, 1, 3).reshape(qkv.shape[0], qkv.shape[1], D)  # noqa: E731
    sa = ((q.abs() / sc) @ k.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    return un(p @ v), dict(p=p, sa=un(sa.expand(-1, -1, -1, hd)), pv=un(p @ v.abs()))


def stage_ln(v, w, b, eps=LN_EPS, ddof=0):
    """LayerNorm over the last dim of v = x + sublayer.  -> (y, (mean, rstd))."""
    if eps == LN_EPS and ddof == 0:
        y = F.layer_norm(v, (v.shape[-1],), w, b, eps)
    else:  # (the fault variants of tests/test_pr_ref_cpu.py)
        m = v.mean(-1, keepdim=True)
        y = (v - m) / torch.sqrt(((v - m) ** 2).sum(-1, keepdim=True) / (v.shape[-1] - ddof) + eps) * w + b
    mean = v.mean(-1)
    var = ((v - mean.unsqueeze(-1)) ** 2).mean(-1)
    return y, (mean, 1.0 / torch.sqrt(var + LN_EPS))


def stage_pool(x, T_div=None):
    return x.sum(1) / (T_div or x.shape[1]), x.abs().mean(1)


def stage_head_compose(w_fc, b_fc, w_head, b_head):
    """Wc = W_head W_fc, bc = W_head b_fc + b_head.  -> ((Wc, bc), (mag Wc, mag bc))."""
    return (w_head @ w_fc, w_head @ b_fc + b_head), (w_head.abs() @ w_fc.abs(), w_head.abs() @ b_fc.abs() + b_head.abs())


def stage_head(pooled, Wc, bc):
    return F.linear(pooled, Wc, bc), F.linear(pooled.abs(), Wc.abs(), bc.abs())


def softplus(vr, branch=True):
    """The kernel's: vr above 20, log1p(exp(vr)) below.  branch=False: the fault - vr everywhere."""
    return torch.where(vr > 20, vr, torch.log1p(torch.exp(vr.clamp(max=20)))) if branch else vr


def stage_sample(head, eps, min_std, branch=True):
    A = head.shape[-1] // 2
    return torch.tanh(head[..., :A] + eps * (softplus(head[..., A:], branch) + min_std))


STAGES = dict(input=stage_input, linear=stage_linear, ffn1=stage_ffn1, ffn2=stage_ffn2, attention=stage_attention, ln=stage_ln,
              pool=stage_pool, head=stage_head, sample=stage_sample)


def forward(P, emb, dtype=torch.float64, rounded=True, stages=None, eps=None):
    """The whole forward in `dtype`, chained from the stages (stages: {name: replacement}, fault injection).  emb (B, T, >= D):
    the first D columns are used.  -> {xin [l], qkv [l], att [l], proj [l], x1 [l], st1 [l], ff1 [l], ff2 [l], st2 [l], out,
    pooled, Wc, bc, head, plan (eps given)}."""
    S = dict(STAGES, **(stages or {}))
    c = lambda t: t.to(dtype)  # noqa: E731
    D = P["pos"].shape[1]
    r = {k: [] for k in ("xin", "qkv", "att", "proj", "x1", "st1", "ff1", "ff2", "st2")}
    x, _ = S["input"](c(emb[..., :D]), c(P["pos"]))
    for Lp in P["layers"]:
        r["xin"].append(x)
        qkv, _ = S["linear"](x, c(Lp["in_w"]), c(Lp["in_b"]), rounded)
        att, _ = S["attention"](qkv)
        proj, _ = S["linear"](att, c(Lp["out_w"]), c(Lp["out_b"]), rounded)
        x1, st1 = S["ln"](x + proj, c(Lp["n1w"]), c(Lp["n1b"]))
        ff1, _ = S["ffn1"](x1, c(Lp["w1"]), c(Lp["b1"]), rounded)
        ff2, _ = S["ffn2"](ff1, c(Lp["w2"]), c(Lp["b2"]), rounded)
        x, st2 = S["ln"](x1 + ff2, c(Lp["n2w"]), c(Lp["n2b"]))
        for k, t in zip(("qkv", "att", "proj", "x1", "st1", "ff1", "ff2", "st2"), (qkv, att, proj, x1, st1, ff1, ff2, st2)):
            r[k].append(t)
    r["out"] = x
    r["pooled"], _ = S["pool"](x)
    (r["Wc"], r["bc"]), _ = stage_head_compose(c(P["fc_w"]), c(P["fc_b"]), c(P["head_w"]), c(P["head_b"]))
    r["head"], _ = S["head"](r["pooled"], r["Wc"], r["bc"])
    if eps is not None:
        r["plan"] = S["sample"](r["head"], c(eps), P["min_std"])
    return r


# ---------------------------------------------------------------------------------------------------- problems
def problem(D, T, FF, L, B, A, ld_emb=None, seed=0, FC=64):
    """Seeded parameters and inputs: {D, T, FF, L, B, A, FC, ld_emb, pos (T, D), layers [l] {LKEYS}, fc_w (FC, D), fc_b,
    head_w (2A, FC) = [mean_fc; variance_fc], head_b, min_std, emb (B, T, ld_emb) fp32, eps (B, A)}.  Weights uniform of variance
    1 / K, LayerNorm weights 1 +- 0.1, biases +- 0.1, emb in [-1, 1] with the pad columns NaN; sequence LOUD is scaled so that its
    layer-0 logits reach ~ LOUD_LOGIT (a peaked softmax), sequence QUIET by 0.25; the first and last variance_fc biases are
    +VAR_BIAS and -VAR_BIAS (A = 1: the one variance row is centred on the batch and scaled until it holds vr beyond +-20 instead).  The
    sequences are the first B of max(B, POP) drawn: a problem's first sequences do not change with B."""
    ld_emb = ld_emb or D
    g = torch.Generator().manual_seed(100003 * seed + 1009 * D + 101 * T + FF + 7 * L)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1  # noqa: E731
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    P = dict(D=D, T=T, FF=FF, L=L, B=B, A=A, FC=FC, ld_emb=ld_emb, min_std=1e-4, layers=[])
    P["pos"] = 0.5 * u(T, D)
    for _ in range(L):
        P["layers"].append(dict(in_w=u(3 * D, D) * math.sqrt(3.0 / D), in_b=0.1 * n(3 * D), out_w=u(D, D) * math.sqrt(3.0 / D),
                                out_b=0.1 * n(D), w1=u(FF, D) * math.sqrt(3.0 / D), b1=0.1 * n(FF),
                                w2=u(D, FF) * math.sqrt(3.0 / FF), b2=0.1 * n(D), n1w=1 + 0.1 * n(D), n1b=0.1 * n(D),
                                n2w=1 + 0.1 * n(D), n2b=0.1 * n(D)))
    P["fc_w"], P["fc_b"] = u(FC, D) * math.sqrt(3.0 / D), 0.1 * n(FC)
    ga = torch.Generator().manual_seed(100003 * seed + 31 * A + 5)  # (the head's draws do not move the encoder's)
    P["head_w"] = (torch.rand(2 * A, FC, generator=ga) * 2 - 1) * math.sqrt(3.0 / FC)
    P["head_b"] = 0.1 * torch.randn(2 * A, generator=ga)
    ge = torch.Generator().manual_seed(100003 * seed + 1009 * D + 101 * T + 3)
    x = (torch.rand(max(B, POP), T, D, generator=ge) * 2 - 1)[:B].clone()
    if B > LOUD:
        Lp = P["layers"][0]
        qkv = (x[LOUD] + P["pos"]).double() @ bf16(Lp["in_w"].double()).t() + Lp["in_b"].double()
        q, k = (_heads(t.unsqueeze(0), D // H) for t in qkv.split(D, dim=-1)[:2])
        top = float(((q @ k.transpose(-1, -2)) / math.sqrt(D // H)).abs().max())
        x[LOUD] *= math.sqrt(LOUD_LOGIT / top)
    if B > QUIET:
        x[QUIET] *= 0.25
    emb = torch.full((B, T, ld_emb), float("nan"))
    emb[..., :D] = x
    P["emb"] = emb
    P["eps"] = torch.randn(max(B, POP), A, generator=torch.Generator().manual_seed(100003 * seed + 77))[:B].clone()
    if A >= 2:
        P["head_b"][A], P["head_b"][2 * A - 1] = VAR_BIAS, -VAR_BIAS
    else:
        P["head_b"][A] = 0.0
        vr = forward(P, emb)["head"][:, A]
        mid = float(vr.median())
        k = VAR_BIAS / max(min(float(vr.max()) - mid, mid - float(vr.min())), 1e-30)
        P["head_w"][A] *= k
        P["head_b"][A] = -k * mid
    return P


def oracle_params(P):
    """The problem under the oracle's (the reference state dict's) names."""
    A = P["A"]
    O = {"position_embeddings.weight": P["pos"], "fc.weight": P["fc_w"], "fc.bias": P["fc_b"],
         "mean_fc.weight": P["head_w"][:A], "mean_fc.bias": P["head_b"][:A],
         "variance_fc.weight": P["head_w"][A:], "variance_fc.bias": P["head_b"][A:]}
    names = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
             "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
             "norm2.bias")
    for l, Lp in enumerate(P["layers"]):
        for k, nm in zip(LKEYS, names):
            O[f"transformer_encoder.layers.{l}.{nm}"] = Lp[k]
    return O


def oracle_head(P, out, dtype, rounded):
    """The oracle's posterior from the encoder output `out` (B, T, D) of forward(): fc on every time step, mean over time, then
    mean_fc | variance_fc, operands rounded where the oracle's _linear rounds them - the oracle does not compose the head, so
    this, not stage_head, is what its (mean, std) are compared with."""
    c = lambda t: t.to(dtype)  # noqa: E731
    A = P["A"]
    x = F.linear(_r(out, rounded), _r(c(P["fc_w"]), rounded), c(P["fc_b"])).mean(1)
    h = F.linear(_r(x, rounded), _r(c(P["head_w"]), rounded), c(P["head_b"]))
    return h[:, :A], F.softplus(h[:, A:]) + P["min_std"]


# ------------------------------------------------------------------------------------------------------ bounds
def ffn2_terms(D, FF):
    """K' of FFN2 from the kernel's structure: a wave accumulates its ceil(nchunk / 4) chunks of `chunk` hidden units in its
    own fp32 MFMA accumulator (started at b2: + 1), then three adds join the partial sums - no element passes through more
    additions.  (<= FF + 4, the count of one sequential sum.)"""
    nchunk = FF // chunk(D)
    return chunk(D) * ((nchunk + 3) // 4) + 1 + 3


def lin_bound(mag, K):
    """A contraction of K' = K terms and extra additions in fp32, any order: |got - ref| <= C_SUM K' U32 (sum |x~||w~| + |b|)."""
    return C_SUM * K * U32 * mag.double()


def att_bound(info, T, hd):
    """|att - ref| per element, the fp32 roundings of pr_fused.hip:274-296 counted to first order.  With Lam = the largest
    sum_e |q_e k_e| / sqrt(hd) over the query's keys (info['sa']):
      logit      the scale constant, the scaling of q, hd products and hd - 1 adds: (hd + 2) U32 sum |q k|, for the key's and for
                 the maximum's logit, and one rounding of s - max (|s - max| <= 2 Lam): <= (2 hd + 6) Lam U32 in the exponent,
                 i.e. relative in 2^x; exp2 itself 1 ulp = 2 U32
      p          numerator and denominator carry that error each; the sum of T positive terms (T - 1) U32, the reciprocal
                 1 ulp = 2 U32, p = e rcp one rounding
      sum p v    T products and adds: (T + 1) U32
    so |err| <= ((4 hd + 12) Lam + 2 T + 8) U32 sum_t p_t |v_t| - logit magnitude x roundings x probability, the form of
    tests/test_seq_gpu.py::_att_scales."""
    return ((4 * hd + 12) * info["sa"].double() + 2 * T + 8) * U32 * info["pv"].double()


def ln_bound(v, w, b):
    """(bound y, bound mean, bound rstd) of layer_norm32_r / layer_norm64 on v = x + sublayer (fp64, exact sum of the two saved
    fp32 tensors), the fp32 roundings of pr_fused.hip:95-117 counted to first order.  depth = D / 4 - 1 + 2 additions at most
    touch a value on its way into a sum (a chain of D / 4 in the lane, two cross-lane adds).
      v     one rounding of the residual add:                       e_v = U32 |v|
      mean  e_m = depth U32 mean|v| + mean e_v  (the division by D is exact)
      c     = v - mean:                                             e_c = e_v + e_m + U32 |c|
      var   = mean c^2: squares one rounding each, the sum `depth`:  e_var = mean(2 |c| e_c) + (depth + 1) U32 var
      rstd  = 1 / sqrtf(var + eps): the add, the root and the division are correctly rounded (hipcc's default):
                                                                    e_r = rstd (e_var / (2 (var + eps)) + 3 U32)
      y     = ((c rstd) w) + b:                                     |w| (e_c rstd + |c| e_r) + 3 U32 |c rstd w| + U32 |y|"""
    v, w, b = v.double(), w.double(), b.double()
    D = v.shape[-1]
    depth = D // 4 - 1 + 2
    mean = v.mean(-1, keepdim=True)
    c = v - mean
    var = (c * c).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    e_v = U32 * v.abs()
    e_m = depth * U32 * v.abs().mean(-1, keepdim=True) + e_v.mean(-1, keepdim=True)
    e_c = e_v + e_m + U32 * c.abs()
    e_var = (2 * c.abs() * e_c).mean(-1, keepdim=True) + (depth + 1) * U32 * var
    e_r = rstd * (e_var / (2 * (var + LN_EPS)) + 3 * U32)
    y = c * rstd * w + b
    e_y = w.abs() * (e_c * rstd + c.abs() * e_r) + 3 * U32 * (c * rstd * w).abs() + U32 * y.abs()
    return e_y, e_m.squeeze(-1), e_r.squeeze(-1)


def pool_bound(y, e_y):
    """pooled = (sum_t y) / T from a y known to e_y: the T - 1 adds (any order; 1 / T is a power of two: exact)."""
    T = y.shape[1]
    return e_y.mean(1) + C_SUM * T * U32 * y.abs().double().mean(1)


def sample_tolerance(head, eps, min_std, level=0.0):
    """plan = tanh(mean + eps (softplus(vr) + min_std)) on the fp32 head: ACT_FACTOR x the worst error of plain fp32 torch -
    on the same head and eps, and (level) on the reference's population of sample_level() -, at least one fp32 ulp of the
    value (mlp_ref.act_tolerance).  -> (reference, tolerance, torch's error)"""
    ref = stage_sample(head.double(), eps.double(), min_std)
    e32 = float((stage_sample(head.float(), eps.float(), min_std).double() - ref).abs().max()) if ref.numel() else 0.0
    e32 = max(e32, level)
    return ref, torch.maximum(torch.full_like(ref, ACT_FACTOR * e32), 2 * U32 * ref.abs()), e32


def sample_level(D, T):
    """Worst error of plain fp32 torch on the plan expression over the reference's own heads and eps of POP sequences at the
    widest latent (POP x 32 elements, from the reference alone).  The worst of the handful of elements one launch of a small
    latent holds does not sample torch's error: seven elements on which torch happens to be exact to a quarter ulp would leave
    the one-ulp floor, which no fp32 tanh of a rounded argument is held to."""
    key = ("sample", D, T)
    if key not in _cache:
        P, f = reference(D, T, 512, 2, POP, A=32)
        _cache[key] = sample_tolerance(f["head"].float(), P["eps"], P["min_std"])[2]
    return _cache[key]


def head_checks(Wc, bc, pooled, head, plan, eps, min_std, level=0.0):
    """H: [(name, reference, per-element bound, torch's fp32 error or None)]: head against fp64 Wc pooled + bc on the kernel's
    own fp32 (Wc, bc, pooled) - a scalar fp32 chain of D products started at bc -, plan against fp64 on the kernel's own head."""
    ref, mag = stage_head(pooled.double(), Wc.double(), bc.double())
    pref, tol, e32 = sample_tolerance(head, eps, min_std, level)
    return [("head", ref, lin_bound(mag, Wc.shape[1] + 1), None), ("plan", pref, tol, e32)]


def stage_checks(P, sv, l):
    """S: [(name, reference, per-element bound)] of layer l, every fp64 stage evaluated on the kernel's OWN saved input (sv:
    {xin, qkv, att, proj, x1, ff1, ff2 (B, T, .), st1, st2 (B, T, 2)} of layer l as fp64), so that one bf16 operand that rounds
    the other way does not cascade.  The LayerNorm-2 output is returned as ('y2', ref, bound): the next layer's xin, or what
    pooled is the time mean of."""
    d = lambda t: t.double()  # noqa: E731
    Lp = {k: d(t) for k, t in P["layers"][l].items()}
    D, T, FF = P["D"], P["T"], P["FF"]
    out = []
    ref, mag = stage_linear(sv["xin"], Lp["in_w"], Lp["in_b"])
    out.append(("qkv", ref, lin_bound(mag, D + 1)))
    ref, info = stage_attention(sv["qkv"])
    out.append(("att", ref, att_bound(info, T, D // H)))
    ref, mag = stage_linear(sv["att"], Lp["out_w"], Lp["out_b"])
    out.append(("proj", ref, lin_bound(mag, D + 1)))
    v = sv["xin"] + sv["proj"]
    ref, (mean, rstd) = stage_ln(v, Lp["n1w"], Lp["n1b"])
    e_y, e_m, e_r = ln_bound(v, Lp["n1w"], Lp["n1b"])
    out += [("x1", ref, e_y), ("st1", torch.stack([mean, rstd], -1), torch.stack([e_m, e_r], -1))]
    ref, mag = stage_ffn1(sv["x1"], Lp["w1"], Lp["b1"])
    out.append(("ff1", ref, lin_bound(mag, D + 1)))
    ref, mag = stage_ffn2(sv["ff1"], Lp["w2"], Lp["b2"])
    out.append(("ff2", ref, lin_bound(mag, ffn2_terms(D, FF))))
    v = sv["x1"] + sv["ff2"]
    ref, (mean, rstd) = stage_ln(v, Lp["n2w"], Lp["n2b"])
    e_y, e_m, e_r = ln_bound(v, Lp["n2w"], Lp["n2b"])
    out += [("st2", torch.stack([mean, rstd], -1), torch.stack([e_m, e_r], -1)), ("y2", ref, e_y)]
    return out


# --------------------------------------------------------------------------------- the end-to-end rule (E2)
_cache = {}


def seq_relerr(got, ref):
    """Per-sequence relative error of a (B, D) pooled tensor (mlp_ref.per_row_relerr)."""
    return per_row_relerr(got, ref)


def reference(D, T, FF, L, B, A=16, ld_emb=None, seed=0):
    """(problem, fully rounded fp64 forward()), computed once."""
    key = ("ref", D, T, FF, L, B, A, ld_emb, seed)
    if key not in _cache:
        P = problem(D, T, FF, L, B, A, ld_emb, seed)
        _cache[key] = (P, forward(P, P["emb"], eps=P["eps"]))
    return _cache[key]


def e2e_population(D, T, FF, L, seed=0, stages=None):
    """e32_b of POP seeded sequences: the fp32 rounded restatement against the fp64 rounded one, per sequence.  The
    distribution is bimodal: most sequences differ by fp32 summation error only, some by a bf16 operand of x, x1 or the
    attention output that rounds the other way."""
    P, ref = reference(D, T, FF, L, POP, seed=seed)
    return seq_relerr(forward(P, P["emb"], torch.float32, stages=stages)["pooled"], ref["pooled"])


def e2e_levels(D, T, FF, L, seed=0):
    """(median, maximum) of the population's e32: what the E2 rule of tests/test_pr_fp64_gpu.py multiplies by E2E_FACTOR."""
    key = ("lv", D, T, FF, L, seed)
    if key not in _cache:
        e = e2e_population(D, T, FF, L, seed)
        _cache[key] = (float(e.median()), float(e.max()))
    return _cache[key]


def e2e_rule(e, levels):
    """E2 on the per-sequence errors e of a launch: the lower quartile <= E2E_FACTOR x the population median, the maximum <=
    E2E_FACTOR x the population maximum.  -> ((quartile, its bound), (max, its bound))."""
    q = float(torch.quantile(e.double(), 0.25))
    return (q, E2E_FACTOR * levels[0]), (float(e.max()), E2E_FACTOR * levels[1])


def e2e_ok(e, levels):
    (q, qb), (m, mb) = e2e_rule(e, levels)
    return q <= qb and m <= mb


# the cases of tests/test_pr_fp64_gpu.py
S_CASES = [(16, 2048, 2, 5, 32), (32, 2048, 2, 3, 32), (16, 256, 1, 3, 36), (16, 1280, 3, 3, 32), (32, 2304, 4, 2, 32),
           (16, 768, 2, 300, 32), (16, 512, 2, 1, 32)]  # (T, FF, L, B, ld_emb), d_model 32
E_CASES = [(32, 2048, 2, 37), (16, 256, 3, 37), (32, 2304, 2, 37), (16, 512, 1, 37)]  # (T, FF, L, B), d_model 64
H_A = [1, 5, 16, 32]
C_CASES = [(D, FC, A2) for D in (32, 64) for FC in (1, 255, 4096) for A2 in (2, 10, 64)]
