"""Conditions on the plan-recognition forward's fp64 reference and on the bounds of tests/test_pr_fp64_gpu.py - nothing here
runs a kernel.  (1) tests/pr_ref.py restates the oracle: its fp32 rounded forward agrees with
oracle.tacorl_oracle.plan_recognition under bf16 operand rounding and its unrounded fp64 forward with the plain oracle, to
fp32 rounding.  (2) The problems discriminate.  (3) A correct fp32 implementation - plain fp32 torch with the kernels'
rounding points, the FFN summed in the kernels' order - stays inside every stage bound and inside the end-to-end rule, so no
bound is tighter than fp32 can meet.  (4) Every planted fault, evaluated in fp32 and checked exactly as the GPU test checks a
kernel (every stage on the faulty run's own saved input), exceeds a stage bound by FAULT_RATIO on at least one element; the
systematic ones violate the end-to-end rule of the d_model-64 kernels, whose levels this file derives and prints."""
import math

import pytest
import torch

from tests import pr_ref as R

F32 = torch.float32


def _uses(P, run):
    """{(stage, layer): worst |got - ref| / bound} of a forward() result checked as test S / H check a launch."""
    out = {}
    x0, _ = R.stage_input(P["emb"][..., :P["D"]], P["pos"])
    out[("xin", 0)] = 0.0 if torch.equal(run["xin"][0].float(), x0) else float("inf")
    for l in range(P["L"]):
        sv = {k: run[k][l].double() for k in ("xin", "qkv", "att", "proj", "x1", "ff1", "ff2")}
        got = dict(sv, st1=torch.stack(run["st1"][l], -1).double(), st2=torch.stack(run["st2"][l], -1).double())
        for name, ref, bound in R.stage_checks(P, sv, l):
            if name == "y2":
                if l + 1 < P["L"]:
                    out[("xin", l + 1)] = R.bound_use(run["xin"][l + 1], ref, bound)
                else:
                    pref, _ = R.stage_pool(ref)
                    out[("pooled", l)] = R.bound_use(run["pooled"], pref, R.pool_bound(ref, bound))
            else:
                out[(name, l)] = R.bound_use(got[name], ref, bound)
    if "plan" in run:
        for name, ref, bound, _ in R.head_checks(run["Wc"].float(), run["bc"].float(), run["pooled"].float(), run["head"].float(),
                                                 run["plan"], P["eps"], P["min_std"], R.sample_level(P["D"], P["T"])):
            out[(name, 0)] = R.bound_use(run[name], ref, bound)
    return out


def _fp32(P, stages=None):
    return R.forward(P, P["emb"], F32, stages=dict({"ffn2": R.stage_ffn2_kernel_order}, **(stages or {})), eps=P["eps"])


@pytest.mark.parametrize("D,T", [(32, 16), (64, 32)])
def test_reference_restates_the_oracle(D, T):
    from oracle import tacorl_oracle as O

    P = R.problem(D, T, 2048, 2, 37, 16)
    OP, emb = R.oracle_params(P), P["emb"][..., :D]
    # without rounding, in fp64: the same function
    f = R.forward(P, emb, torch.float64, rounded=False)
    mu, sd = O.plan_recognition({k: v.double() for k, v in OP.items()}, "", emb.double(), min_std=P["min_std"])
    rmu, rsd = R.oracle_head(P, f["out"], torch.float64, False)
    e64 = (R.relerr(mu, rmu), R.relerr(sd, rsd))
    # with bf16 operand rounding, both in fp32: the same operations on the same rounded operands - per sequence, so that one
    # sequence that is off cannot hide in the norm
    f = R.forward(P, emb, F32, rounded=True)
    with O.operand_rounding(torch.bfloat16):
        mu, sd = O.plan_recognition(OP, "", emb, min_std=P["min_std"])
    rmu, rsd = R.oracle_head(P, f["out"], F32, True)
    e32 = (float(R.seq_relerr(rmu, mu).max()), float(R.seq_relerr(rsd, sd).max()))
    # the composed head is the same affine map as fc -> mean_fc | variance_fc
    h = R.forward(P, emb, torch.float64, rounded=False)
    ec = R.relerr(h["head"][:, :16], R.oracle_head(P, h["out"], torch.float64, False)[0])
    print(D, T, "fp64 unrounded", e64, "fp32 rounded, worst sequence", e32, "composed head", ec)
    assert max(e64) < 1e-12 and ec < 1e-12, (e64, ec)
    assert max(e32) <= 16 * R.U32, e32  # fp32 rounding: no operand rounds the other way between two runs of the same fp32 operations


@pytest.mark.parametrize("D,T", [(32, 16), (32, 32), (64, 16), (64, 32)])
def test_problems_are_discriminating(D, T):
    P, f = R.reference(D, T, 512, 2, 37, A=5, ld_emb=D + 4)
    assert torch.isnan(P["emb"][..., D:]).all() and torch.isfinite(P["emb"][..., :D]).all()
    assert torch.equal(R.problem(D, T, 512, 2, 5, 5, D + 4)["emb"][..., :D], P["emb"][:5, :, :D])  # the first sequences do not change with B
    pos = P["pos"]
    assert float(torch.cdist(pos, pos).add(torch.eye(T) * 9).min()) > 0.5, "position rows are distinct"
    hd = D // R.H
    q, k = (R._heads(t, hd) for t in f["qkv"][0].split(D, dim=-1)[:2])
    logit = ((q @ k.transpose(-1, -2)) / math.sqrt(hd)).abs().amax((1, 2, 3))
    assert 20 < float(logit[R.LOUD]) < 45 and float(logit[0]) < 10, logit[:3]
    assert float(f["att"][0].abs().max()) > 0 and float(R.stage_attention(f["qkv"][0])[1]["p"][R.LOUD].max()) > 0.99  # a peaked softmax
    on = (f["ff1"][0] > 0).double().mean((0, 1))
    assert 0.02 < float(on.median()) < 0.98
    for A in R.H_A:
        Pa, fa = R.reference(D, T, 512, 2, 37, A=A)
        vr = fa["head"][:, A:]
        assert bool((vr > 20).any()) and bool((vr < -20).any()) and bool((vr.abs() < 5).any() or A < 3), (A, vr.min(), vr.max())


CPU_CASES = [(32, 16, 2048, 2, 5), (32, 32, 2304, 4, 2), (32, 16, 1280, 3, 3), (32, 16, 256, 1, 3), (64, 32, 2048, 2, 3), (64, 16, 256, 3, 3)]


@pytest.mark.parametrize("D,T,FF,L,B", CPU_CASES)
def test_fp32_stays_inside_every_stage_bound(D, T, FF, L, B):
    P, _ = R.reference(D, T, FF, L, B, A=5)
    use = _uses(P, _fp32(P))
    worst = max(use.items(), key=lambda kv: kv[1])
    print((D, T, FF, L, B), "worst use of a bound", worst, {k: f"{v:.2g}" for k, v in use.items() if k[1] == 0})
    assert worst[1] <= 1.0, {k: v for k, v in use.items() if v > 1.0}


# ------------------------------------------------------------------------------------------------ planted faults
def _trunc(t):
    """bf16 by truncation."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(t.dtype)


def _lin_trunc(x, W, b, rounded=True):
    return F_linear(_trunc(x), R.bf16(W), b), None


def F_linear(x, W, b):
    return torch.nn.functional.linear(x, W, b)


def _ffn1_trunc(x, W, b, rounded=True):
    return torch.relu(F_linear(_trunc(x), R.bf16(W), b)), None


def _ffn2_with(edit):
    def f(h, W2, b2, rounded=True):
        h, W2, b2 = edit(R.bf16(h).clone(), R.bf16(W2).clone(), b2)
        return R.stage_ffn2_kernel_order(h, W2, b2, rounded=False)
    return f


def _ffn2_hidden_trunc(h, W2, b2, rounded=True):
    return R.stage_ffn2_kernel_order(_trunc(h), R.bf16(W2), b2, rounded=False)


def _drop_unit(h, W2, b2):
    j = int(((h.abs().amax((0, 1))) * W2.abs().amax(0)).argmax())
    h[..., j] = 0
    return h, W2, b2


def _drop_chunk(h, W2, b2):
    CH = R.chunk(W2.shape[0])
    h[..., -CH:] = 0
    return h, W2, b2


def _att_last_key(qkv):
    att, info = R.stage_attention(qkv)
    D = qkv.shape[-1] // 3
    hd = D // R.H
    q, k, v = (R._heads(t, hd) for t in qkv.split(D, dim=-1))
    s = (q[0, 3, 5] / math.sqrt(hd)) @ k[0, 3, :-1].t()
    att = att.clone()
    att[0, 5, 3 * hd: 4 * hd] = torch.softmax(s, -1) @ v[0, 3, :-1]
    return att, info


def _att_swap_heads(qkv):
    att, info = R.stage_attention(qkv)
    hd = qkv.shape[-1] // 3 // R.H
    a = att.clone()
    a[..., 2 * hd: 3 * hd], a[..., 5 * hd: 6 * hd] = att[..., 5 * hd: 6 * hd], att[..., 2 * hd: 3 * hd]
    return a, info


def _att_wrong_hd(qkv):
    hd = qkv.shape[-1] // 3 // R.H
    return R.stage_attention(qkv, hd_scale=12 - hd)  # (the other kernel's head dimension: 4 <-> 8)


def _pos_shift(emb, pos):
    return emb + pos[torch.arange(emb.shape[1]) % 16], None


def _sample_eps_neighbour(head, eps, min_std):
    return R.stage_sample(head, eps.roll(1, 0), min_std)


FAULTS = {  # name: (stages replaced, systematic: it enters pooled on every sequence, so it must also violate the end-to-end rule)
    "bf16 truncation of the projections' operand": ({"linear": _lin_trunc}, True),
    "bf16 truncation of x1": ({"ffn1": _ffn1_trunc}, True),
    "bf16 truncation of the hidden state": ({"ffn2": _ffn2_hidden_trunc}, True),
    "one hidden unit left out of FFN2": ({"ffn2": _ffn2_with(_drop_unit)}, True),
    "one chunk left out of FFN2": ({"ffn2": _ffn2_with(_drop_chunk)}, True),
    "b2 added four times": ({"ffn2": _ffn2_with(lambda h, W, b: (h, W, 4 * b))}, True),
    "last key left out of one query": ({"attention": _att_last_key}, False),  # (one query of one sequence: 6e-4 .. 9e-4 of that
    # sequence's pooled row - a bf16 operand that rounds the other way does as much, so only a per-stage check can see it)
    "two heads swapped": ({"attention": _att_swap_heads}, True),
    "1/sqrt(hd) of the wrong head dimension": ({"attention": _att_wrong_hd}, True),
    "LayerNorm without eps": ({"ln": lambda v, w, b: R.stage_ln(v, w, b, eps=0.0)}, True),
    "LayerNorm with D - 1": ({"ln": lambda v, w, b: R.stage_ln(v, w, b, ddof=1)}, True),
    "position row t used for t + 16": ({"input": _pos_shift}, True),
    "pooled divided by 16": ({"pool": lambda x: R.stage_pool(x, T_div=16)}, True),
    "softplus without the log1p(exp) branch": ({"sample": lambda h, e, m: R.stage_sample(h, e, m, branch=False)}, False),
    "eps of the neighbouring sequence": ({"sample": _sample_eps_neighbour}, False),
}
T32_ONLY = ("position row t used for t + 16", "pooled divided by 16")


@pytest.mark.parametrize("D,T,name", [(D, T, n) for D, T in ((32, 16), (32, 32), (64, 32)) for n in FAULTS
                                      if T == 32 or n not in T32_ONLY])
def test_planted_fault_exceeds_a_stage_bound(D, T, name):
    P, _ = R.reference(D, T, 2048, 2, 5, A=5)
    use = _uses(P, _fp32(P, FAULTS[name][0]))
    worst = max(use.items(), key=lambda kv: kv[1])
    print(f"{name} (D {D}, T {T}): worst use of a bound {worst[1]:.3g} at {worst[0]}")
    assert worst[1] >= R.FAULT_RATIO, (name, worst)


# ---------------------------------------------------------------------------------------- the end-to-end rule (E2)
@pytest.mark.parametrize("T,FF,L,B", R.E_CASES)
def test_end_to_end_rule_calibration(T, FF, L, B):
    """The levels of E2 (d_model 64), derived here: the population's e32 median and maximum, how many sequences sit above
    10 x the median (a bf16 operand that rounds the other way), and what removing every rounding would give.  A second valid
    fp32 evaluation (the kernels' FFN order) of the B sequences the GPU test launches satisfies the rule; each systematic
    fault violates it."""
    D = 64
    lv = R.e2e_levels(D, T, FF, L)
    e = R.e2e_population(D, T, FF, L)
    Pp, refp = R.reference(D, T, FF, L, R.POP)
    unr = R.seq_relerr(R.forward(Pp, Pp["emb"], F32, rounded=False)["pooled"], refp["pooled"])
    print(f"d_model 64 {(T, FF, L)}: e32 median {lv[0]:.2e}, max {lv[1]:.2e}, above 10 x median {int((e > 10 * lv[0]).sum())} of {R.POP};"
          f" without any rounding: median {float(unr.median()):.2e}")
    assert 0 < lv[0] < lv[1] < 2.0 ** -8
    assert not R.e2e_ok(unr[:B], lv), ("dropping every rounding must violate the rule", R.e2e_rule(unr[:B], lv))
    P, ref = R.reference(D, T, FF, L, B)
    assert torch.equal(P["emb"], Pp["emb"][:B])
    ok = R.seq_relerr(_fp32(P)["pooled"], ref["pooled"])
    print("   kernel-order fp32:", R.e2e_rule(ok, lv))
    assert R.e2e_ok(ok, lv), R.e2e_rule(ok, lv)
    for name, (stages, enc) in FAULTS.items():
        if not enc or (name in T32_ONLY and T != 32):
            continue
        bad = R.seq_relerr(_fp32(P, stages)["pooled"], ref["pooled"])
        print(f"   {name}:", R.e2e_rule(bad, lv))
        assert not R.e2e_ok(bad, lv), (name, R.e2e_rule(bad, lv))
