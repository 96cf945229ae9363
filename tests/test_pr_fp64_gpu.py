"""The one-launch plan-recognition forward (tacorl_amd/csrc/pr_fused.hip: pr_encoder_fused_kernel<1|2>,
pr_encoder_fused64_kernel<1|2>, pr_head_compose_kernel) stage by stage and element by element against the fp64
restatement of tests/pr_ref.py, through the C entry points themselves, at the shapes where the kernels take another path:
waves without a chunk, an uneven chunk split, the unstaged FFN1 bias, 1 / 3 / 4 layers, a padded input pitch, one sequence,
more workgroups than CUs, latent sizes 1, 5, 16 and 32.

  S  d_model 32, train-mode launch: every saved tensor of every layer against the fp64 stage evaluated on the kernel's OWN
     saved input (xin[0] = emb + pos bit for bit), pooled from the last layer's saves; NaN-filled buffers, guard tails
  I  the inference launch writes the train launch's pooled, bit for bit
  H  head and plan of the _sample launches from the kernel's own pooled / head, both softplus branches; pooled and the saves
     bit-identical to the launch without the head
  C  tacorl_pr_head_compose against fp64, and its refusals
  E  d_model 64 (no saves): E1 a sequence's pooled row does not depend on where or with whom it is launched (also d_model
     32); E2 the per-sequence error against the fully rounded fp64 forward under the rule of pr_ref.e2e_rule
  R  the refusals of the forward launcher come before any launch

Every bound comes from tests/pr_ref.py (tests/test_pr_ref_cpu.py shows what the bounds still detect); every measured number
goes to golden_util.record_margin (tools/pr_margins_md.py -> profiles/pr_forward_margins.md).  A test collects all its
figures before it asserts."""
import ctypes as C

import pytest
import torch

from tests import pr_ref as R
from tests.golden_util import record_margin

pytestmark = pytest.mark.gpu

EINVAL = -22
NAN = float("nan")
TAIL = 64  # floats of NaN guard behind every output buffer
SAVE_KEYS = ("xin", "qkv", "att", "proj", "x1", "ff1", "ff2", "st1", "st2")  # PrSaveL order


def _dev():
    from tacorl_amd import _lib

    _lib.call("tacorl_hip_init", 0)
    return torch.device("cuda:0")


def _buf(n, dev):
    return torch.full((n + TAIL,), NAN, device=dev)


class _Net:
    """Problem P on the device: the fp32 parameter block (every tensor at a multiple of 4 elements), its bf16 mirror from
    tacorl_to_bf16_batch, the offsets array of the launcher and the composed head of tacorl_pr_head_compose."""

    def __init__(self, P):
        from tacorl_amd import _lib

        self.dev = dev = _dev()
        self.P = P
        ts = [P["pos"]] + [Lp[k] for Lp in P["layers"] for k in R.LKEYS] + [P["fc_w"], P["fc_b"], P["head_w"], P["head_b"]]
        offs, n = [], 0
        for t in ts:
            offs.append(n)
            n += (t.numel() + 3) // 4 * 4
        flat = torch.zeros(n + TAIL)
        for o, t in zip(offs, ts):
            flat[o: o + t.numel()] = t.reshape(-1)
        self.flat = flat.to(dev)
        self.pb = torch.zeros(n + TAIL, dtype=torch.bfloat16, device=dev)
        _lib.call("tacorl_to_bf16_batch", 1, _lib.ptr_array([self.flat]), _lib.ptr_array([self.pb]), (C.c_long * 1)(n + TAIL),
                  _lib.stream())
        self.offsets = offs[: 1 + 12 * P["L"]]
        self.foff = (C.c_long * len(self.offsets))(*self.offsets)
        D, A, FC = P["D"], P["A"], P["FC"]
        self.Wc, self.bc = _buf(2 * A * D, dev), _buf(2 * A, dev)
        h = offs[1 + 12 * P["L"]:]
        p = lambda o: C.c_void_p(self.flat.data_ptr() + 4 * o)  # noqa: E731
        _lib.call("tacorl_pr_head_compose", p(h[0]), p(h[1]), p(h[2]), p(h[3]), _lib.ptr(self.Wc), _lib.ptr(self.bc), D, FC, 2 * A,
                  _lib.stream())
        torch.cuda.synchronize()
        self.mirror_ok = torch.equal(self.pb, self.flat.to(torch.bfloat16))  # RNE of the fp32 block, bit for bit

    def launch(self, mode, emb=None, eps=None):
        """mode: plain | train | sample | train_sample.  -> {pooled (B, D), head, plan, sv [l] {SAVE_KEYS} (cpu), tails: every
        guard tail still NaN}."""
        from tacorl_amd import _lib

        P, dev = self.P, self.dev
        D, T, FF, L, A = P["D"], P["T"], P["FF"], P["L"], P["A"]
        emb = (P["emb"] if emb is None else emb).to(dev).contiguous()
        B, ld = emb.shape[0], emb.shape[2]
        eps = (P["eps"] if eps is None else eps).to(dev).contiguous()
        pooled, head, plan = _buf(B * D, dev), _buf(B * 2 * A, dev), _buf(B * A, dev)
        sizes = dict(xin=D, qkv=3 * D, att=D, proj=D, x1=D, ff1=FF, ff2=D, st1=2, st2=2)
        sv = [{k: _buf(B * T * sizes[k], dev) for k in SAVE_KEYS} for _ in range(L)]
        save = _lib.ptr_array([s[k] for s in sv for k in SAVE_KEYS])
        base = (_lib.ptr(emb), ld, _lib.ptr(self.flat), _lib.ptr(self.pb), self.foff, _lib.ptr(pooled), B, D, T, R.H, FF, L)
        smp = (_lib.ptr(self.Wc), _lib.ptr(self.bc), _lib.ptr(eps), _lib.ptr(head), _lib.ptr(plan), A, float(P["min_std"]))
        if mode == "plain":
            _lib.call("tacorl_pr_encoder_fused", *base, _lib.stream())
        elif mode == "train":
            _lib.call("tacorl_pr_encoder_fused_train", *base, save, _lib.stream())
        elif mode == "sample":
            _lib.call("tacorl_pr_encoder_fused_sample", *base, *smp, _lib.stream())
        else:
            _lib.call("tacorl_pr_encoder_fused_train_sample", *base, save, *smp, _lib.stream())
        torch.cuda.synchronize()
        bufs = [pooled, head, plan] + [s[k] for s in sv for k in SAVE_KEYS]
        out = dict(tails=all(bool(torch.isnan(t[-TAIL:]).all()) for t in bufs), pooled=pooled[:-TAIL].view(B, D).cpu(),
                   head=head[:-TAIL].view(B, 2 * A).cpu(), plan=plan[:-TAIL].view(B, A).cpu())
        out["sv"] = [{k: s[k][:-TAIL].view(B, T, sizes[k]).cpu() for k in SAVE_KEYS} for s in sv]
        return out


_runs = {}


def _train_run(case):
    """The train-mode launch of an S case, once: (net, outputs)."""
    if case not in _runs:
        T, FF, L, B, ld = case
        P, _ = R.reference(32, T, FF, L, B, A=16, ld_emb=ld)
        net = _Net(P)
        _runs[case] = (net, net.launch("train"))
    return _runs[case]


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.isfinite(a).all()) and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ S, I
@pytest.mark.parametrize("case", R.S_CASES, ids=lambda c: "T%d_FF%d_L%d_B%d_ld%d" % c)
def test_train_launch_every_saved_tensor_per_stage(case):
    T, FF, L, B, ld = case
    net, out = _train_run(case)
    P = net.P
    tag = "T%d FF%d L%d B%d ld%d" % case
    x0, _ = R.stage_input(P["emb"][..., :32], P["pos"])
    facts = {"bf16 mirror is RNE of the block": net.mirror_ok, "guard tails untouched": out["tails"],
             "xin[0] == emb + pos bit for bit": _same_bits(out["sv"][0]["xin"], x0),
             "head / plan untouched": _all_nan(out["head"]) and _all_nan(out["plan"])}
    use = {}
    for l in range(L):
        sv = {k: out["sv"][l][k].double() for k in SAVE_KEYS}
        for name, ref, bound in R.stage_checks(P, sv, l):
            if name == "y2" and l + 1 < L:
                name, got = f"xin[{l + 1}]", out["sv"][l + 1]["xin"]
            elif name == "y2":
                pref, _ = R.stage_pool(ref)
                name, got, ref, bound = "pooled", out["pooled"], pref, R.pool_bound(ref, bound)
            else:
                got, name = sv[name], f"{name}[{l}]"
            use[name] = R.bound_use(got, ref, bound)
            record_margin(f"{tag} {name}", use[name], 1.0, kind="S err / bound")
    print(tag, {k: f"{v:.2g}" for k, v in use.items()}, facts)
    assert all(facts.values()), facts
    assert max(use.values()) <= 1.0, {k: v for k, v in use.items() if v > 1.0}


@pytest.mark.parametrize("case", R.S_CASES, ids=lambda c: "T%d_FF%d_L%d_B%d_ld%d" % c)
def test_inference_launch_equals_train_launch(case):
    net, out = _train_run(case)
    inf = net.launch("plain")
    assert inf["tails"] and all(_all_nan(s[k]) for s in inf["sv"] for k in SAVE_KEYS) and _all_nan(inf["head"])
    assert _same_bits(inf["pooled"], out["pooled"])


# --------------------------------------------------------------------------------------------------------------- H
@pytest.mark.parametrize("A", R.H_A)
@pytest.mark.parametrize("D,T", [(32, 16), (32, 32), (64, 16), (64, 32)])
def test_head_and_sample_from_the_kernels_own_pooled(D, T, A):
    B = 7
    P, _ = R.reference(D, T, 512, 2, B, A=A)
    net = _Net(P)
    tag = f"D{D} T{T} A{A}"
    s = net.launch("sample")
    plain = net.launch("plain")
    Wc, bc = net.Wc[:-TAIL].view(2 * A, D).cpu(), net.bc[:-TAIL].cpu()
    vr = s["head"][:, A:]
    facts = {"guard tails untouched": s["tails"] and plain["tails"] and _all_nan(net.Wc[-TAIL:]) and _all_nan(net.bc[-TAIL:]),
             "vr > 20 and vr < -20 occur": bool((vr > 20).any()) and bool((vr < -20).any()),
             "pooled == the launch without the head": _same_bits(s["pooled"], plain["pooled"])}
    runs = [("sample", s)]
    if D == 32:
        ts, t = net.launch("train_sample"), net.launch("train")
        facts["train_sample: pooled, saves == train"] = ts["tails"] and _same_bits(ts["pooled"], t["pooled"]) and all(
            _same_bits(a[k], b[k]) for a, b in zip(ts["sv"], t["sv"]) for k in SAVE_KEYS)
        facts["train pooled == inference pooled"] = _same_bits(t["pooled"], plain["pooled"])
        runs.append(("train_sample", ts))
    use = {}
    for entry, r in runs:
        for name, ref, bound, e32 in R.head_checks(Wc, bc, r["pooled"], r["head"], r["plan"], P["eps"], P["min_std"],
                                                   R.sample_level(D, T)):
            use[(entry, name)] = R.bound_use(r[name], ref, bound)
            record_margin(f"{tag} {entry} {name}", use[(entry, name)], 1.0, floor=e32, kind="H err / bound")
    print(tag, {k: f"{v:.2g}" for k, v in use.items()}, facts)
    assert all(facts.values()), facts
    assert max(use.values()) <= 1.0, use


# --------------------------------------------------------------------------------------------------------------- C
def _compose_inputs(D, FC, A2, dev):
    g = torch.Generator().manual_seed(1000 * D + 10 * FC + A2)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1  # noqa: E731
    return [t.to(dev) for t in (u(FC, D), u(FC), u(A2, FC), u(A2))]


@pytest.mark.parametrize("D,FC,A2", R.C_CASES)
def test_head_compose(D, FC, A2):
    from tacorl_amd import _lib

    dev = _dev()
    ins = _compose_inputs(D, FC, A2, dev)
    Wc, bc = _buf(A2 * D, dev), _buf(A2, dev)
    _lib.call("tacorl_pr_head_compose", *[_lib.ptr(t) for t in ins], _lib.ptr(Wc), _lib.ptr(bc), D, FC, A2, _lib.stream())
    torch.cuda.synchronize()
    (rW, rb), (mW, mb) = R.stage_head_compose(*[t.double().cpu() for t in ins])
    uW = R.bound_use(Wc[:-TAIL].view(A2, D), rW, R.lin_bound(mW, FC))
    ub = R.bound_use(bc[:-TAIL], rb, R.lin_bound(mb, FC + 1))
    record_margin(f"D{D} FC{FC} A2_{A2} Wc", uW, 1.0, kind="C err / bound")
    record_margin(f"D{D} FC{FC} A2_{A2} bc", ub, 1.0, kind="C err / bound")
    print((D, FC, A2), "Wc", uW, "bc", ub)
    assert _all_nan(Wc[-TAIL:]) and _all_nan(bc[-TAIL:])
    assert uW <= 1.0 and ub <= 1.0, (uW, ub)


def test_head_compose_refusals():
    from tacorl_amd import _lib

    dev = _dev()
    D, FC, A2 = 32, 8, 4
    ins = _compose_inputs(D, FC, A2, dev)
    Wc, bc = _buf(A2 * D, dev), _buf(A2, dev)
    fn = _lib.lib().tacorl_pr_head_compose
    ptrs = [_lib.ptr(t) for t in ins] + [_lib.ptr(Wc), _lib.ptr(bc)]
    rcs = {"D = 48": fn(*ptrs, 48, FC, A2, _lib.stream()), "FC = 0": fn(*ptrs, D, 0, A2, _lib.stream()),
           "A2 = 0": fn(*ptrs, D, FC, 0, _lib.stream())}
    for k in range(6):
        rcs[f"null pointer {k}"] = fn(*[None if j == k else p for j, p in enumerate(ptrs)], D, FC, A2, _lib.stream())
    torch.cuda.synchronize()
    assert all(rc == EINVAL for rc in rcs.values()), rcs
    assert _all_nan(Wc) and _all_nan(bc)


# --------------------------------------------------------------------------------------------------------------- E
def _e1(net, full):
    """A sequence's pooled row whatever the launch: alone, first, last (the batch reversed), in a batch of another size."""
    P = net.P
    B = P["B"]
    facts = {}
    if B > 1:
        rev = net.launch("plain", emb=P["emb"].flip(0))
        facts["reversed batch"] = rev["tails"] and _same_bits(rev["pooled"].flip(0), full["pooled"])
        n = min(5, B - 1)
        part = net.launch("plain", emb=P["emb"][B - n:])
        facts["batch of another size"] = _same_bits(part["pooled"], full["pooled"][B - n:])
    for j in sorted({0, min(R.LOUD, B - 1), B - 1}):
        one = net.launch("plain", emb=P["emb"][j: j + 1])
        facts[f"sequence {j} alone"] = one["tails"] and _same_bits(one["pooled"], full["pooled"][j: j + 1])
    return facts


@pytest.mark.parametrize("case", R.E_CASES, ids=lambda c: "T%d_FF%d_L%d_B%d" % c)
def test_d_model_64_end_to_end(case):
    T, FF, L, B = case
    P, ref = R.reference(64, T, FF, L, B)
    net = _Net(P)
    tag = "D64 T%d FF%d L%d B%d" % case
    full = net.launch("plain")
    facts = dict(_e1(net, full), **{"guard tails untouched": full["tails"], "bf16 mirror is RNE of the block": net.mirror_ok})
    facts["sample launch: same pooled"] = _same_bits(net.launch("sample")["pooled"], full["pooled"])
    e = R.seq_relerr(full["pooled"], ref["pooled"])
    lv = R.e2e_levels(64, T, FF, L)
    (q, qb), (m, mb) = R.e2e_rule(e, lv)
    record_margin(f"{tag} lower quartile", q, qb, floor=lv[0], kind="E2 per sequence")
    record_margin(f"{tag} worst sequence", m, mb, floor=lv[1], kind="E2 per sequence")
    print(tag, f"lower quartile {q:.3g} <= {qb:.3g}, worst {m:.3g} <= {mb:.3g}, median {float(e.median()):.3g}", facts)
    assert all(facts.values()), facts
    assert bool(torch.isfinite(full["pooled"]).all()) and q <= qb and m <= mb, ((q, qb), (m, mb))


@pytest.mark.parametrize("case", [c for c in R.S_CASES if c[3] <= 5], ids=lambda c: "T%d_FF%d_L%d_B%d_ld%d" % c)
def test_d_model_32_row_does_not_depend_on_the_launch(case):
    net, out = _train_run(case)
    facts = _e1(net, out)
    assert all(facts.values()), facts


# --------------------------------------------------------------------------------------------------------------- R
def test_forward_launcher_refusals():
    """Every call returns TACORL_EINVAL and leaves pooled, head, plan and every save buffer NaN.  (Views one float / two bf16
    further into a buffer with a guard tail are the 4-byte misalignments: in bounds whatever a launch would do.)"""
    from tacorl_amd import _lib

    lib = _lib.lib()
    D, T, FF, L, B, A = 32, 16, 512, 2, 3, 16
    P, _ = R.reference(D, T, FF, L, B, A=A)
    net = _Net(P)
    dev = net.dev
    P64, _ = R.reference(64, T, FF, L, B, A=A)
    net64 = _Net(P64)
    emb, emb64 = P["emb"].to(dev).reshape(-1), P64["emb"].to(dev).reshape(-1)
    emb = torch.cat([emb, torch.zeros(TAIL, device=dev)])
    eps = P["eps"].to(dev).contiguous()
    pooled, head, plan = _buf(B * 64, dev), _buf(B * 2 * 33, dev), _buf(B * 33, dev)
    sizes = dict(xin=D, qkv=3 * D, att=D, proj=D, x1=D, ff1=FF, ff2=D, st1=2, st2=2)
    svb = [_buf(B * T * 2 * sizes[k], dev) for _ in range(R.MAXL + 1) for k in SAVE_KEYS]
    st = _lib.stream()

    def args(**o):
        a = dict(emb=_lib.ptr(emb), ld=D, params=_lib.ptr(net.flat), pb=_lib.ptr(net.pb), off=net.foff, pooled=_lib.ptr(pooled), B=B, D=D,
                 T=T, H=R.H, FF=FF, L=L, save=_lib.ptr_array(svb[: 9 * L]), Wc=_lib.ptr(net.Wc), bc=_lib.ptr(net.bc), eps=_lib.ptr(eps),
                 head=_lib.ptr(head), plan=_lib.ptr(plan), A=A, min_std=1e-4)
        a.update(o)
        return a

    def base(a):
        return (a["emb"], a["ld"], a["params"], a["pb"], a["off"], a["pooled"], a["B"], a["D"], a["T"], a["H"], a["FF"], a["L"])

    def smp(a):
        return (a["Wc"], a["bc"], a["eps"], a["head"], a["plan"], a["A"], a["min_std"])

    entries = {"plain": lambda a: lib.tacorl_pr_encoder_fused(*base(a), st),
               "train": lambda a: lib.tacorl_pr_encoder_fused_train(*base(a), a["save"], st),
               "sample": lambda a: lib.tacorl_pr_encoder_fused_sample(*base(a), *smp(a), st),
               "train_sample": lambda a: lib.tacorl_pr_encoder_fused_train_sample(*base(a), a["save"], *smp(a), st)}
    off1 = lambda t, k=1: C.c_void_p(t.data_ptr() + 4 * k)  # noqa: E731  (4 k bytes further)
    bad_off = lambda i: (C.c_long * len(net.offsets))(*[o + (1 if j == i else 0) for j, o in enumerate(net.offsets)])  # noqa: E731
    long_off = (C.c_long * (1 + 12 * 5))(*(net.offsets + net.offsets[1:13] * 3))
    sv_with = lambda i, v: _lib.ptr_array([v if j == i else t for j, t in enumerate(svb[: 9 * L])])  # noqa: E731
    every = ("plain", "train", "sample", "train_sample")
    cases = [("D = 48", every, dict(D=48)), ("T = 8", every, dict(T=8)), ("T = 48", every, dict(T=48)), ("H = 4", every, dict(H=4)),
             ("FF = 128", every, dict(FF=128)), ("FF = 2176", every, dict(FF=2176)), ("L = 0", every, dict(L=0)),
             ("L = 5", every, dict(L=5, off=long_off, save=_lib.ptr_array(svb[: 45]))), ("ld_emb = 34", every, dict(ld=34)),
             ("B = 0", every, dict(B=0)), ("emb + 4 bytes", every, dict(emb=off1(emb))), ("params + 4 bytes", every, dict(params=off1(net.flat))),
             ("params_bf16 + 4 bytes", every, dict(pb=off1(net.pb))), ("pooled + 4 bytes", every, dict(pooled=off1(pooled))),
             ("Wc + 4 bytes", ("sample", "train_sample"), dict(Wc=off1(net.Wc))),
             ("position offset + 1", every, dict(off=bad_off(0))), ("in_proj_weight offset + 1", every, dict(off=bad_off(1))),
             ("layer 1 norm2.bias offset + 1", every, dict(off=bad_off(24))),
             ("A = 0", ("sample", "train_sample"), dict(A=0)), ("A = 33", ("sample", "train_sample"), dict(A=33)),
             ("null save pointer", ("train", "train_sample"), dict(save=sv_with(5, None))),
             ("last save pointer null", ("train", "train_sample"), dict(save=sv_with(9 * L - 1, None))),
             ("save pointer + 4 bytes", ("train", "train_sample"), dict(save=sv_with(10, off1(svb[10])))),
             ("save = NULL", ("train", "train_sample"), dict(save=None)),
             ("Wc = NULL", ("sample", "train_sample"), dict(Wc=None)),
             ("bc = NULL", ("sample", "train_sample"), dict(bc=None)), ("eps = NULL", ("sample", "train_sample"), dict(eps=None)),
             ("head = NULL", ("sample", "train_sample"), dict(head=None)), ("plan = NULL", ("sample", "train_sample"), dict(plan=None)),
             ("save with d_model 64", ("train", "train_sample"), dict(D=64, ld=64, emb=_lib.ptr(emb64), params=_lib.ptr(net64.flat),
                                                                       pb=_lib.ptr(net64.pb), off=net64.foff, Wc=_lib.ptr(net64.Wc),
                                                                       bc=_lib.ptr(net64.bc)))]
    rcs = {}
    for name, which, o in cases:
        for e in which:
            rcs[(name, e)] = entries[e](args(**o))
    sup = lib.tacorl_pr_encoder_fused_supported
    supported = {"32 16": sup(32, 16, 8, 256, 1), "64 32": sup(64, 32, 8, 2304, 4), "train 64": lib.tacorl_pr_encoder_fused_train_supported(64, 16, 8, 512, 2),
                 "train 32": lib.tacorl_pr_encoder_fused_train_supported(32, 32, 8, 512, 2), "48": sup(48, 16, 8, 512, 2), "L5": sup(32, 16, 8, 512, 5)}
    torch.cuda.synchronize()
    wrong = {k: v for k, v in rcs.items() if v != EINVAL}
    assert not wrong, wrong
    assert supported == {"32 16": 1, "64 32": 1, "train 64": 0, "train 32": 1, "48": 0, "L5": 0}, supported
    assert all(_all_nan(t) for t in [pooled, head, plan] + svb), "a refused call wrote to an output"
