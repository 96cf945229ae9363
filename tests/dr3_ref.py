"""The DR3 term of the critics restated in plain torch (reference modules/cql/cql_offline_lightning.py:424-437, 496-499),
its gradient, and the a-priori bounds the GPU tests hold tacorl_dr3_fwd_bwd to.  Nothing here runs a kernel.

The term, per critic, with emb_obs = enc(obs) (B, Eo) carrying the gradient and emb_next = enc(next_obs) (B, Eo) a constant:

    v = coef / B * sum_b sum_j emb_obs[b, j] * emb_next[b, j]              (value)
    d emb_obs[b, j] += T[b, j],   T = coef * gs / B * emb_next[b, j]       (gs = 1 / world: the per-rank scale)

The coefficient reaches the kernel as an fp32 launch argument, so every reference below starts from float32(coef).

Bounds, with u = 2^-24 (fp32 unit round-off) and N = B * Eo.

Value.  Each product is rounded once: fl(o n) = o n (1 + d), |d| <= u.  A sum of N terms, in ANY order, passes each term
through at most N - 1 rounded additions, so |fl(sum) - sum o n| <= ((1 + u)^N - 1) * sum |o n| including the products'
roundings.  The factor coef / B is formed once in fp64 and rounded to fp32 (one rounding), the final multiplication is one
more: (1 + u)^(N + 2) - 1 = (N + 2) u to first order.  Hence

    |v_kernel - v_fp64| <= (N + 2) * u * coef / B * sum |o n|.

The second-order remainder, (N + 2)^2 u^2 / 2, is 5e-4 of the bound at the largest N here (257 * 64); the kernel's own
summation tree is ceil(N / 256) + 9 additions deep, not N - 1, so the first-order statement has two orders of magnitude to
spare where N is large and is exact to first order where N is small.

Gradient element.  s = fl(coef * gs / B) is one rounding of a product formed in fp64, t = fl(s * n) a second, and the add
d' = fl(d + t) a third, relative to |d + t|:  |d' - (d + T)| <= 2u |T| + u (|d| + |T|) + O(u^2) <= 3u (|d| + |T|).
The O(u^2) remainder (3 u^2 |T|) is covered by the slack 2u |d| as soon as |d| > 2u |T|; the tests pre-fill d with
magnitudes in [0.25, 1), never zero.

    |d_kernel - (d_before + T)| <= 3 * u * (|d_before| + |T|)      per element.
"""
import numpy as np
import torch

U = 2.0 ** -24
PAD = 1.0e30  # fills the columns >= Eo of the operand rows: a kernel that reads them cannot stay inside a bound


def f32(x):
    """The fp32 value a float launch argument carries."""
    return float(np.float32(x))


def dr3_loss(emb_obs, emb_next, coef):
    """The reference's expression (cql_offline_lightning.py:428-429) - differentiable in emb_obs, in emb_obs's dtype."""
    return (emb_obs * emb_next.detach()).sum(dim=1).mean(dim=0) * coef


def value(obs, nxt, coef, dtype=torch.float64):
    o, n = obs.to(dtype), nxt.to(dtype)
    return float((o * n).sum() * (f32(coef) / o.shape[0]))


def grad_term(nxt, coef, gs, dtype=torch.float64):
    """T = coef * gs / B * emb_next."""
    return nxt.to(dtype) * (f32(coef) * f32(gs) / nxt.shape[0])


def value_bound(obs, nxt, coef):
    B, Eo = obs.shape
    return (B * Eo + 2) * U * f32(coef) / B * float((obs.double() * nxt.double()).abs().sum())


def grad_bound(d_before, nxt, coef, gs):
    return 3.0 * U * (d_before.double().abs() + grad_term(nxt, coef, gs).abs())


def problem(B, Eo, ld, seed, n=2):
    """Operands of one launch over n critics: per critic obs, next (B, ld) with the first Eo columns the data and PAD behind,
    d (B, ld) pre-filled everywhere.  Magnitudes in [0.25, 1); next alternates its sign by column (both signs in the
    gradient), the product obs * next is negative in every fourth column and positive elsewhere - so no row sum, column sum
    or total is a cancellation, and dropping any single row or column moves the value by far more than its bound."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * B + Eo + ld)
    mag = lambda *s: torch.rand(*s, generator=g) * 0.75 + 0.25  # noqa: E731
    j = torch.arange(Eo)
    s_next = torch.where(j % 2 == 0, 1.0, -1.0)
    s_obs = s_next * torch.where(j % 4 == 3, -1.0, 1.0)
    out = []
    for _ in range(n):
        obs, nxt = torch.full((B, ld), PAD), torch.full((B, ld), PAD)
        obs[:, :Eo], nxt[:, :Eo] = mag(B, Eo) * s_obs, mag(B, Eo) * s_next
        d = mag(B, ld) * torch.where(torch.rand(B, ld, generator=g) < 0.5, -1.0, 1.0)
        out.append(dict(obs=obs, next=nxt, d=d))
    return out


def golden_embeddings(g, P, step=0):
    """{critic: (enc(obs), enc(next_obs))} over the observation cameras of a golden's batch, by the oracle's encoder forward
    on the parameters P (inside oracle.operand_rounding the contractions round their operands as the bf16 kernels do)."""
    from oracle import tacorl_oracle as O

    batch, cams = g.batch(step), sorted(g.cams)
    if g.cfg["kind"] == "tacorl":  # get_rl_batch (tacorl.py:142-179): s = states[:, 0], s' = states[:, -1]
        obs = {c: v[:, 0] for c, v in batch["states"].items()}
        nxt = {c: v[:, -1] for c, v in batch["states"].items()}
    else:
        obs, nxt = batch["observations"]["observation"], batch["next_observations"]["observation"]
    return {k: (O.late_fusion(P, f"{k}.encoder.", obs, cams), O.late_fusion(P, f"{k}.encoder.", nxt, cams)) for k in ("q1", "q2")}


def golden_terms(g, P, step=0):
    """({critic: value of its DR3 term}, {parameter name: gradient of the term}) by autograd through the oracle's encoder
    forward: what has to be added to the oracle's step, which knows nothing of DR3.  P is not modified."""
    coef = g.cfg["overrides"]["dr3_coefficient"]
    vals, grads = {}, {}
    for k, (eo, en) in golden_embeddings(g, P, step).items():
        loss = dr3_loss(eo, en, coef)
        names = [n for n in P if n.startswith(f"{k}.encoder.") and P[n].requires_grad]
        gs = torch.autograd.grad(loss, [P[n] for n in names], allow_unused=True)
        vals[k] = float(loss.detach())
        grads.update({n: gr for n, gr in zip(names, gs) if gr is not None})
    return vals, grads
