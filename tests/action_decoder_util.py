"""A plain-torch restatement of the action decoder's loss (2-layer ReLU nn.RNN over [plan | emb_t], four logistic-mixture
heads, oracle.tacorl_oracle.logistic_mixture_loss) for the tests of tacorl_amd/networks/action_decoder.py: the loss, the heads
and hidden states in the module's layouts, and autograd gradients with respect to the RNN's input rows and every parameter.

It is oracle.action_decoder_fwd written out - the same `_linear` calls in the same order, so `operand_rounding(bf16)` applies
and the fp64 values are equal (tests/test_action_decoder_cpu.py) - with ONE difference, the ReLU rule of `_ReluFollows` in
tests/test_seq_gpu.py: every ReLU is z * gate, gate = (z > 0) of the restatement itself, except at ties
|z| < TIE_REL * mean|z| (the mean over that layer's pre-activations), where a caller-supplied decision (the module's own
h_l > 0) is taken: a pre-activation within fp32 rounding of zero may land on either side, and the side decides a whole
hidden unit's gradient.  A supplied decision that differs AWAY from a tie is an error of the module and raises."""
import torch

from oracle import tacorl_oracle as O
from tacorl_amd.synth import param_values

TIE_REL = 1e-4   # a tie: |z| below this share of the layer's mean |z|
TIE_CAP = 1e-3   # share of tied gates per layer a test may rely on (measured with the reference alone: <= 1.3e-4)
HEADS = ("mean_fc", "log_scale_fc", "prob_fc", "gripper_fc")  # the module's head order: [means | log_scales | logit_probs | gripper]


def param_shapes(H, In, L, n_mix=10, Da=6):
    """{reference name: shape} of ActionDecoderLogistic (rnn_decoder, discrete gripper)."""
    s = {}
    for l in range(L):
        s[f"rnn.weight_ih_l{l}"] = (H, In if l == 0 else H)
        s[f"rnn.weight_hh_l{l}"] = (H, H)
        s[f"rnn.bias_ih_l{l}"] = (H,)
        s[f"rnn.bias_hh_l{l}"] = (H,)
    for n in HEADS:
        rows = 2 if n == "gripper_fc" else Da * n_mix
        s[n + ".weight"], s[n + ".bias"] = (rows, H), (rows,)
    return s


def make_params(H, In, L, seed):
    """Deterministic weights (synth.param_values: U(+-1/sqrt(fan_in))), biases scaled by 3 so that none of them is negligible."""
    return {k: param_values(k, shp, seed) * (3.0 if "bias" in k else 1.0) for k, shp in param_shapes(H, In, L).items()}


def make_inputs(B, Tm, P, E, seed, T=None):
    """plan (B,P), frame embeddings (B,T,E), actions (B,T,7) of a window of T >= Tm frames (default Tm + 1: the decoder is
    trained on all but the last).  Actions: randn clamped to +-1 - about 30 % of the entries sit ON the bounds (the loss's
    edge branches), the others inside (the cdf-difference branch) - and a gripper column of +-1."""
    T = Tm + 1 if T is None else T
    g = torch.Generator().manual_seed(seed)
    plan, emb = torch.randn(B, P, generator=g), torch.randn(B, T, E, generator=g)
    acts = torch.randn(B, T, 7, generator=g).clamp(-1, 1)
    acts[..., 6] = torch.where(acts[..., 6] >= 0, 1.0, -1.0)
    return plan, emb, acts


def decoder_loss(W, plan, emb, actions, dtype=torch.float64, L=2, n_mix=10, num_classes=10, gripper_alpha=1.0, gates=None,
                 strict=True, rounded=False, grad=True):
    """W {reference name: tensor}; plan (B,P); emb (B,Tm,E); actions (B,Tm,7).  gates: per layer a bool (Tm,B,H) - the
    decisions taken at ties (None: the restatement's own everywhere); strict: a supplied decision that differs away from a
    tie raises.  rounded: contractions with bf16 operands (oracle.operand_rounding; dtype must be float32).
    Returns a dict: loss; heads (Tm*B, NH) and h [L x (Tm,B,H)] in the module's sequence-major layouts; dx_seq (Tm*B, P+E) =
    d loss / d [plan | emb_t] per input row; grads {name: d loss / d W[name]} (bias_ih and bias_hh separately); ties [share
    of tied gates per layer]; disagree [share of supplied decisions that differ away from a tie, per layer: 0 when strict];
    gates [the decisions used, L x (Tm,B,H) bool]."""
    assert not rounded or dtype == torch.float32
    B, Tm, _ = emb.shape
    Wd = {k: v.detach().to(dtype).clone().requires_grad_(grad) for k, v in W.items()}
    x = torch.cat([plan.unsqueeze(1).expand(-1, Tm, -1), emb], dim=-1).detach().to(dtype).clone().requires_grad_(grad)

    def rnn(gate_of):
        inp, hs = x, []
        for l in range(L):
            wi, wh = Wd[f"rnn.weight_ih_l{l}"], Wd[f"rnn.weight_hh_l{l}"]
            bi, bh = Wd[f"rnn.bias_ih_l{l}"], Wd[f"rnn.bias_hh_l{l}"]
            h = torch.zeros(B, wh.shape[0], dtype=dtype)
            xin = O._linear(inp, wi, bi)
            outs = []
            for t in range(Tm):
                z = xin[:, t] + O._linear(h, wh, bh)
                h = z * gate_of(l, t, z.detach()).to(dtype)
                outs.append(h)
            inp = torch.stack(outs, dim=1)
            hs.append(inp)
        return hs

    def run():
        # pass 1 (no gradient, plain ReLU): the mean |z| of every layer, which sets that layer's tie threshold
        zsum = [0.0] * L

        def plain(l, t, z):
            zsum[l] += float(z.abs().sum())
            return z > 0

        with torch.no_grad():
            H = rnn(plain)[0].shape[-1]
        thr = [TIE_REL * s / (B * Tm * H) for s in zsum]
        used = [[None] * Tm for _ in range(L)]
        nties, ndiff = [0] * L, [0] * L

        def follow(l, t, z):
            own = z > 0
            if gates is not None:
                tie = z.abs() < thr[l]
                theirs = gates[l][t]
                if strict and bool((theirs != own)[~tie].any()):
                    bad = ((theirs != own) & ~tie).nonzero()[0].tolist()
                    raise AssertionError(f"layer {l} step {t}: the module's ReLU decision differs away from a tie, first at "
                                         f"(b, unit) = {bad}: z = {z[tuple(bad)].item():.3g}, tie below {thr[l]:.3g}")
                nties[l] += int(tie.sum())
                ndiff[l] += int(((theirs != own) & ~tie).sum())
                own = torch.where(tie, theirs, own)
            else:
                nties[l] += int((z.abs() < thr[l]).sum())
            used[l][t] = own
            return own

        hs = rnn(follow)
        top = hs[-1]
        head = {n: O._linear(top, Wd[n + ".weight"], Wd[n + ".bias"]) for n in ("prob_fc", "mean_fc", "log_scale_fc", "gripper_fc")}
        v = lambda t: t.reshape(B, Tm, -1, n_mix)  # noqa: E731
        loss = O.logistic_mixture_loss(v(head["prob_fc"]), v(torch.clamp(head["log_scale_fc"], min=O.LOG_SIG_MIN)),
                                       v(head["mean_fc"]), head["gripper_fc"], actions.to(dtype), num_classes, gripper_alpha)
        share = lambda c: [n / (B * Tm * H) for n in c]  # noqa: E731
        return loss, head, hs, (share(nties), share(ndiff)), [torch.stack(u) for u in used]

    if rounded:
        with O.operand_rounding(torch.bfloat16):
            loss, head, hs, ties, used = run()
    else:
        loss, head, hs, ties, used = run()
    seq = lambda t: t.detach().transpose(0, 1).reshape(Tm * B, -1)  # noqa: E731  (B,Tm,*) -> rows t*B + b
    out = {"loss": loss.detach(), "heads": seq(torch.cat([head[n] for n in HEADS], dim=-1)),
           "h": [h.detach().transpose(0, 1).contiguous() for h in hs], "ties": ties[0], "disagree": ties[1], "gates": used}
    if grad:
        loss.backward()
        out["dx_seq"] = seq(x.grad)
        out["grads"] = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in Wd.items()}
    return out


def flat(res):
    """One {name: tensor} of everything a restatement (or a module run in the same form) is compared on."""
    d = {"loss": res["loss"], "heads": res["heads"], "dx_seq": res["dx_seq"]}
    d.update({f"h{l}": h for l, h in enumerate(res["h"])})
    d.update(res["grads"])
    return d


def is_forward(name):
    return name in ("loss", "heads") or (name[0] == "h" and name[1:].isdigit())


_FLOORS = {}


def rounded_floor(W, plan, emb, actions, L, base, key=None):
    """Reproducibility of the bf16-rounded restatement itself (golden_util.gradient_floor, here over the forward quantities
    too): `base` = decoder_loss(..., float32, rounded=True) re-evaluated with every weight perturbed by one fp32 ulp, ties
    frozen to base's gates.  {name: worst relative change}; no bf16 kernel can be held tighter.  key: memoise.
    Under "gate disagreement": per layer, the largest share of ReLU decisions of a perturbed run that differ from base's away
    from a tie - two evaluations whose hidden states are rounded to bf16 separately do not take the same decisions, and this is
    how often the restatement itself does not (GATE_DISAGREE in the GPU test)."""
    from tests.golden_util import gradient_floor

    if key is not None and key in _FLOORS:
        return _FLOORS[key]

    differ = [0.0] * L

    def again(Pp):
        r = decoder_loss(Pp, plan, emb, actions, torch.float32, L=L, gates=base["gates"], strict=False, rounded=True)
        differ[:] = [max(a, b) for a, b in zip(differ, r["disagree"])]
        return flat(r)

    fl = gradient_floor(again, {k: v.detach() for k, v in W.items()}, flat(base))
    fl["gate disagreement"] = differ
    if key is not None:
        _FLOORS[key] = fl
    return fl
