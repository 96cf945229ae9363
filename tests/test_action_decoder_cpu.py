"""What makes the reference of tests/test_action_decoder_gpu.py trustworthy, without a GPU: the restatement
(tests/action_decoder_util.py) equals the oracle's action_decoder_fwd + logistic_mixture_loss in fp64, its autograd gradients
equal central differences of its own loss, and its tie rule stays within the cap the GPU tests rely on."""
import pytest
import torch

from oracle import tacorl_oracle as O
from tests.action_decoder_util import TIE_CAP, decoder_loss, make_inputs, make_params

# (B, Tm, H, P, E, L): the f32 cases of the GPU test
CASES = [(5, 6, 128, 16, 32, 2), (37, 5, 35, 14, 32, 2), (64, 3, 256, 16, 32, 3), (16, 1, 128, 16, 32, 2), (8, 4, 128, 16, 32, 1)]


def _case(B, Tm, H, P, E, L):
    W = make_params(H, P + E, L, seed=B + Tm + H)
    plan, emb, acts = make_inputs(B, Tm, P, E, seed=B * Tm + H)
    return W, plan, emb[:, :Tm], acts[:, :Tm]


@pytest.mark.parametrize("B,Tm,H,P,E,L", CASES)
def test_restatement_equals_oracle_fp64(B, Tm, H, P, E, L):
    """Loss, heads and hidden states against oracle.action_decoder_fwd + logistic_mixture_loss to 1e-12 (same expressions in
    the same order: only z * (z > 0) in place of relu(z)), the layouts the module uses, and the tie statistics: the fp32
    restatement never decides a gate differently from fp64 away from a tie, and at most TIE_CAP of a layer's gates are tied."""
    W, plan, emb, acts = _case(B, Tm, H, P, E, L)
    r = decoder_loss(W, plan, emb, acts, torch.float64, L=L)
    W64 = {k: v.double() for k, v in W.items()}
    lp, ls, mm, gr, hn = O.action_decoder_fwd(W64, "", plan.double(), emb.double(), n_layers=L, return_hidden=True)
    loss = O.logistic_mixture_loss(lp, ls, mm, gr, acts.double())
    assert abs(float(r["loss"]) - float(loss)) <= 1e-12 * abs(float(loss))
    DK = 60
    heads = r["heads"].view(Tm, B, -1).transpose(0, 1)  # rows t*B + b -> (B, Tm, NH)
    assert heads.shape[-1] == 3 * DK + 2
    for got, ref in ((heads[..., :DK], mm), (heads[..., DK:2 * DK].clamp(min=O.LOG_SIG_MIN), ls), (heads[..., 2 * DK:3 * DK], lp),
                     (heads[..., 3 * DK:], gr)):
        assert (got.reshape(ref.shape) - ref).abs().max() <= 1e-12 * ref.abs().max()
    for l in range(L):
        assert r["h"][l].shape == (Tm, B, H)
        assert (r["h"][l][Tm - 1] - hn[l]).abs().max() <= 1e-12 * hn[l].abs().max().clamp_min(1e-300)
    assert set(r["grads"]) == set(W) and r["dx_seq"].shape == (Tm * B, P + E)
    for l in range(L):  # the two biases enter as a sum (autograd adds their rows in different orders: not bit-equal)
        gi, gh = r["grads"][f"rnn.bias_ih_l{l}"], r["grads"][f"rnn.bias_hh_l{l}"]
        assert (gi - gh).abs().max() <= 1e-12 * gi.abs().max()
    if Tm == 1:  # W_hh only ever multiplies the zero state
        assert all(float(r["grads"][f"rnn.weight_hh_l{l}"].abs().max()) == 0.0 for l in range(L))
    # the fp32 restatement, given fp64's decisions at ties, must agree with them everywhere else (strict raises otherwise)
    r32 = decoder_loss(W, plan, emb, acts, torch.float32, L=L, gates=r["gates"], strict=True, grad=False)
    print(f"B{B}/Tm{Tm}/H{H}/L{L}: tied share per layer {['%.3g' % t for t in r32['ties']]}")
    assert max(r["ties"]) <= TIE_CAP and max(r32["ties"]) <= TIE_CAP


def test_restatement_follows_supplied_gates_only_at_ties():
    """A supplied decision is taken at a tie and refused away from one."""
    B, Tm, H, P, E, L = 5, 3, 35, 14, 32, 2
    W, plan, emb, acts = _case(B, Tm, H, P, E, L)
    r = decoder_loss(W, plan, emb, acts, torch.float64, L=L, grad=False)
    flipped = [g.clone() for g in r["gates"]]
    flipped[1][1, 2, 3] = ~flipped[1][1, 2, 3]
    with pytest.raises(AssertionError, match="differs away from a tie"):
        decoder_loss(W, plan, emb, acts, torch.float64, L=L, gates=flipped, grad=False)
    again = decoder_loss(W, plan, emb, acts, torch.float64, L=L, gates=r["gates"], grad=False)
    assert torch.equal(again["loss"], r["loss"])


@pytest.mark.parametrize("B,Tm,H,P,E,L", [(5, 6, 128, 16, 32, 2), (37, 5, 35, 14, 32, 2)])
def test_restatement_gradients_are_central_differences(B, Tm, H, P, E, L):
    """d loss / d W[name][i] by autograd against (loss(W + e) - loss(W - e)) / 2e in fp64, gates frozen to the unperturbed
    run's (the loss is piecewise smooth; e = 1e-6 keeps every perturbed pre-activation on its side except at a tie), at
    three entries of every parameter and of the input rows.  Bound: the difference quotient's own error - e^2 |f'''| / 6,
    negligible, plus the loss's fp64 rounding (~1e-15 * |loss| ~ 1e-14) over 2e = 5e-9 - hence 1e-7 absolute + 1e-6 relative."""
    W, plan, emb, acts = _case(B, Tm, H, P, E, L)
    r = decoder_loss(W, plan, emb, acts, torch.float64, L=L)
    W64 = {k: v.double() for k, v in W.items()}
    e = 1e-6
    gen = torch.Generator().manual_seed(3)

    def loss_at(Wp, plan_=plan.double(), emb_=emb.double()):
        return float(decoder_loss(Wp, plan_, emb_, acts, torch.float64, L=L, gates=r["gates"], strict=False, grad=False)["loss"])

    for name, g in r["grads"].items():
        for _ in range(3):
            i = int(torch.randint(g.numel(), (1,), generator=gen))
            d = torch.zeros(g.numel(), dtype=torch.float64)
            d[i] = e
            d = d.view(g.shape)
            fd = (loss_at({**W64, name: W64[name] + d}) - loss_at({**W64, name: W64[name] - d})) / (2 * e)
            ad = float(g.flatten()[i])
            assert abs(fd - ad) <= 1e-7 + 1e-6 * abs(ad), (name, i, fd, ad)
    # an embedding entry: row t*B + b of dx_seq, column P + j; a plan entry: the sum over t of rows t*B + b, column j
    dx = r["dx_seq"].view(Tm, B, P + E)
    for b, t, j in ((0, 0, 0), (B - 1, Tm - 1, E - 1), (B // 2, Tm // 2, 5)):
        d = torch.zeros_like(emb, dtype=torch.float64)
        d[b, t, j] = e
        fd = (loss_at(W64, emb_=emb.double() + d) - loss_at(W64, emb_=emb.double() - d)) / (2 * e)
        assert abs(fd - float(dx[t, b, P + j])) <= 1e-7 + 1e-6 * abs(fd), ("emb", b, t, j)
        d = torch.zeros_like(plan, dtype=torch.float64)
        d[b, j % P] = e
        fd = (loss_at(W64, plan_=plan.double() + d) - loss_at(W64, plan_=plan.double() - d)) / (2 * e)
        assert abs(fd - float(dx[:, b, j % P].sum())) <= 1e-7 + 1e-6 * abs(fd), ("plan", b, j % P)
