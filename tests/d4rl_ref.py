"""Plain-torch restatement of the reference's vector-observation (D4RL) steps - modules/play_lmp/play_lmp_d4rl.py,
modules/cql/cql_offline_lightning_d4rl.py, modules/tacorl/tacorl_d4rl.py - with every random draw an explicit input.  It runs
in whatever dtype its parameter dict P holds (fp32 to reproduce the goldens, fp64 as the GPU tests' reference) and under
oracle.tacorl_oracle.operand_rounding (the MFMA's bf16 operand rounding): every contraction goes through the oracle's
`_linear`.  The policy, Q network, tanh-Gaussian log-probabilities, plan-recognition transformer, balanced KL, Adam and
gradient clipping are the oracle's own functions; what is stated here is what the D4RL modules do differently from the image
ones - no encoder in front of any network, the decoder without a gripper head - and the step around it.

Parameter names are the reference's state-dict keys: `actor.policy.*`, `q1.Q.*`, `target_q1.Q.*`, `plan_recognition.*`,
`action_decoder.*`, `log_alpha`, `log_alpha_prime` (TACORL); `plan_proposal.policy.*` (PlayLMP)."""
import math

import torch
import torch.nn.functional as F

from oracle import tacorl_oracle as O
from oracle.tacorl_oracle import LOG_SIG_MIN, _REGION, _expand, _grads, _linear, group_names, policy, qnet, tanh_logprob

GOAL_DIM = 2


# ------------------------------------------------------------------ action decoder, discrete_gripper: False
def action_decoder_fwd(P, pre, plan, emb, n_mix=10, n_layers=2):
    """ActionDecoderLogistic.forward (action_decoder_logistic.py:268-300) without gripper_fc (:293): logit_probs, log_scales,
    means (B, T, Da, n_mix)."""
    B, T, _ = emb.shape
    x = torch.cat([plan.unsqueeze(1).expand(-1, T, -1), emb], dim=-1)
    _REGION.append("rnn")
    for l in range(n_layers):
        wi, wh = P[f"{pre}rnn.weight_ih_l{l}"], P[f"{pre}rnn.weight_hh_l{l}"]
        bi, bh = P[f"{pre}rnn.bias_ih_l{l}"], P[f"{pre}rnn.bias_hh_l{l}"]
        h = torch.zeros(B, wh.shape[0], dtype=emb.dtype)
        xin = _linear(x, wi, bi)
        outs = []
        for t in range(T):
            h = F.relu(xin[:, t] + _linear(h, wh, bh))
            outs.append(h)
        x = torch.stack(outs, dim=1)
    probs = _linear(x, P[pre + "prob_fc.weight"], P[pre + "prob_fc.bias"])
    means = _linear(x, P[pre + "mean_fc.weight"], P[pre + "mean_fc.bias"])
    log_scales = torch.clamp(_linear(x, P[pre + "log_scale_fc.weight"], P[pre + "log_scale_fc.bias"]), min=LOG_SIG_MIN)
    _REGION.pop()
    v = lambda t: t.reshape(B, T, -1, n_mix)  # noqa: E731
    return v(probs), v(log_scales), v(means)


def logistic_loss(logit_probs, log_scales, means, actions, num_classes=10):
    """_loss with discrete_gripper False (:134-138) = _logistic_loss (:184-235) over every action dimension, bounds +-1."""
    a = actions.unsqueeze(-1)
    log_scales = torch.clamp(log_scales, min=LOG_SIG_MIN)
    centered, inv_std = a - means, torch.exp(-log_scales)
    half_bin = 1.0 / (num_classes - 1)
    plus_in, min_in, mid_in = inv_std * (centered + half_bin), inv_std * (centered - half_bin), inv_std * centered
    cdf_delta = torch.sigmoid(plus_in) - torch.sigmoid(min_in)
    log_pdf_mid = mid_in - log_scales - 2.0 * F.softplus(mid_in)
    a_b = a.expand_as(means)
    log_probs = torch.where(
        a_b < -1.0 + 1e-3, plus_in - F.softplus(plus_in),
        torch.where(a_b > 1.0 - 1e-3, -F.softplus(min_in),
                    torch.where(cdf_delta > 1e-5, torch.log(torch.clamp(cdf_delta, min=1e-12)),
                                log_pdf_mid - math.log((num_classes - 1) / 2))))
    log_probs = log_probs + F.log_softmax(logit_probs, dim=-1)
    m = log_probs.max(dim=-1, keepdim=True).values  # utils/misc.py:289-294
    lse = m.squeeze(-1) + torch.log(torch.exp(log_probs - m).sum(dim=-1))
    return -lse.sum(dim=-1).mean()


def logistic_sample(logit_probs, log_scales, means, rand_a, rand_b):
    """_sample (:238-266) without the gripper command: (B, T, Da)."""
    r1, r2 = 1e-5, 1.0 - 1e-5
    t = logit_probs - torch.log(-torch.log((r1 - r2) * rand_a + r2))
    dist = F.one_hot(torch.argmax(t, -1), logit_probs.shape[-1]).to(means.dtype)
    u = (r1 - r2) * rand_b + r2
    return (dist * means).sum(-1) + torch.exp((dist * log_scales).sum(-1)) * (torch.log(u) - torch.log(1.0 - u))


# ------------------------------------------------------------------ CQL update on vector rows
class Spec:
    """What the reference module reads from its config (config/module/tacorl_d4rl.yaml) and from the environment."""

    def __init__(self, n=4, discount=0.95, tau=0.005, actor_lr=1e-4, critic_lr=3e-4, deterministic_backup=True,
                 reward_scale=10.0, bc_epochs=0, clip_grad_val=1.0, conservative_weight=1.0, lagrange_thresh=5.0, temp=1.0,
                 with_lagrange=True, target_entropy=-8.0, finetune_action_decoder=False, action_decoder_lr=3e-4):
        self.__dict__.update(locals())
        del self.__dict__["self"]


def ac_update(P, opts, spec, obs, next_obs, action, rewards, dones, noise, epoch, logs):
    """CQL_Offline.compute_update (cql_offline_lightning_d4rl.py:388-460).  obs / next_obs (B, state + goal) rows, rewards /
    dones (B,1); noise: eps_pi, eps_next (B,A), u_rand (nB,A) U(0,1), eps_cur, eps_nxt (n,B,A).  Every gradient is taken on
    the pre-step graph (no loss reads a parameter that an earlier optimiser step of the iteration moved - except alpha, which
    is read after its step, :374).  Mutates P; returns the gradients by name."""
    n, B = spec.n, action.shape[0]
    dt = action.dtype
    rd, one_minus_d = rewards.to(dt), (1 - dones).to(dt)
    out = {}
    mu, std = policy(P, "actor.policy.", obs)
    z = mu + noise["eps_pi"] * std
    cur_a, log_pi = torch.tanh(z), tanh_logprob(z, mu, std)
    alpha_loss = -(P["log_alpha"][0] * (log_pi + spec.target_entropy).detach()).mean()
    g = _grads(alpha_loss, P, ["log_alpha"])
    out.update(g)
    opts["alpha"].step(P, g)
    alpha = P["log_alpha"][0].exp()
    logs["alpha"] = alpha.item()
    if epoch < spec.bc_epochs:
        actor_loss = (alpha * log_pi - O.tanh_logprob_of_value(action, mu, std)).mean()
    else:
        actor_loss = (alpha * log_pi - torch.min(qnet(P, "q1.Q.", obs, cur_a), qnet(P, "q2.Q.", obs, cur_a))).mean()
    with torch.no_grad():  # compute_critic_loss :202-232
        mn, sn = policy(P, "actor.policy.", next_obs)
        zn = mn + noise["eps_next"] * sn
        nxt_a, nxt_lp = torch.tanh(zn), tanh_logprob(zn, mn, sn)
        qn = torch.min(qnet(P, "target_q1.Q.", next_obs, nxt_a), qnet(P, "target_q2.Q.", next_obs, nxt_a))
        if not spec.deterministic_backup:
            qn = qn - alpha * nxt_lp
        y = spec.reward_scale * rd + one_minus_d * spec.discount * qn
    q1_data, q2_data = qnet(P, "q1.Q.", obs, action), qnet(P, "q2.Q.", obs, action)
    bell1, bell2 = F.mse_loss(q1_data, y), F.mse_loss(q2_data, y)
    A = cur_a.shape[-1]  # compute_conservative_loss :234-324
    rand_a = noise["u_rand"] * 2.0 - 1.0
    rand_density = math.log(0.5 ** A)
    obs_n = _expand(obs, n)

    def q_both(acts_flat):
        return (qnet(P, "q1.Q.", obs_n, acts_flat).view(n, B).transpose(0, 1),
                qnet(P, "q2.Q.", obs_n, acts_flat).view(n, B).transpose(0, 1))

    def sample_n(m_, s_, eps):
        with torch.no_grad():
            zz = m_.unsqueeze(0) + eps * s_.unsqueeze(0)
            return torch.tanh(zz).reshape(-1, A), tanh_logprob(zz, m_, s_).squeeze(-1).transpose(0, 1)

    q1_rand, q2_rand = q_both(rand_a)
    a_cur, lp_cur = sample_n(mu.detach(), std.detach(), noise["eps_cur"])
    a_nxt, lp_nxt = sample_n(mn, sn, noise["eps_nxt"])
    q1_cur, q2_cur = q_both(a_cur)
    q1_nxt, q2_nxt = q_both(a_nxt)
    logs.update(q1_data=q1_data.mean().item(), q1_random=q1_rand.mean().item(), q1_policy=q1_cur.mean().item(),
                q2_data=q2_data.mean().item(), q2_random=q2_rand.mean().item(), q2_policy=q2_cur.mean().item())
    cat1 = torch.cat([q1_rand - rand_density, q1_cur - lp_cur, q1_nxt - lp_nxt], dim=1)
    cat2 = torch.cat([q2_rand - rand_density, q2_cur - lp_cur, q2_nxt - lp_nxt], dim=1)
    w, temp = spec.conservative_weight, spec.temp
    cons1 = torch.logsumexp(cat1 / temp, dim=1).mean() * w * temp - q1_data.mean() * w
    cons2 = torch.logsumexp(cat2 / temp, dim=1).mean() * w * temp - q2_data.mean() * w
    if spec.with_lagrange:
        alpha_p = torch.clamp(P["log_alpha_prime"][0].exp(), min=0.0, max=1000000.0)
        logs["alpha_prime"] = alpha_p.item()
        cons1, cons2 = alpha_p * (cons1 - spec.lagrange_thresh), alpha_p * (cons2 - spec.lagrange_thresh)
        ap_loss = (-cons1 - cons2) * 0.5
        logs["alpha_prime_loss"] = ap_loss.item()
        out.update(_grads(ap_loss, P, ["log_alpha_prime"]))
    q1_loss, q2_loss = bell1 + cons1, bell2 + cons2
    logs.update(bellman_q1_loss=bell1.item(), conservative_q1_loss=cons1.item(), q1_loss=q1_loss.item(),
                bellman_q2_loss=bell2.item(), conservative_q2_loss=cons2.item(), q2_loss=q2_loss.item(),
                actor_loss=actor_loss.item(), alpha_loss=alpha_loss.item())
    an, q1n, q2n = group_names(P, "actor."), group_names(P, "q1."), group_names(P, "q2.")
    ga, g1, g2 = _grads(actor_loss, P, an), _grads(q1_loss, P, q1n), _grads(q2_loss, P, q2n, retain=False)
    if spec.with_lagrange:
        opts["alpha_prime"].step(P, {"log_alpha_prime": out["log_alpha_prime"]})
    for names, gg, key in ((an, ga, "actor"), (q1n, g1, "q1"), (q2n, g2, "q2")):
        out.update({k: v.clone() for k, v in gg.items()})
        O.clip_grads_(gg, names, spec.clip_grad_val)
        opts[key].step(P, gg)
    with torch.no_grad():  # soft_update_from_to :151-154
        for src, dst in (("q1.", "target_q1."), ("q2.", "target_q2.")):
            for nme in group_names(P, src):
                t = P[dst + nme[len(src):]]
                t.copy_(t * (1.0 - spec.tau) + P[nme] * spec.tau)
    return out


def require_grad_(P):
    """TACORL: the plan recognition and the target critics have no gradient (tacorl_d4rl.py:66; targets are Polyak copies)."""
    return O.require_grad_(P, frozen_prefixes=("plan_recognition.", "target_q1.", "target_q2."))


def tacorl_step(P, opts, spec, batch, noise, epoch, optimize=True):
    """TACORL.training_step (tacorl_d4rl.py:141-160); optimize=False: the validation sequence (no parameter moves).
    Returns (logs, latent plan, gradients by name)."""
    logs, grads = {}, {}
    obs, acts = batch["observations"], batch["actions"]
    dt = P["log_alpha"].dtype
    obs, acts, goal = obs.to(dt), acts.to(dt), batch["goal"].to(dt)
    with torch.no_grad():  # get_pr_latent_plan :134-139 (eval mode: no dropout)
        mu, std = O.plan_recognition(P, "plan_recognition.", obs)
        plan = torch.tanh(mu + noise["eps_pr"].to(dt) * std)
    lp, ls, mm = action_decoder_fwd(P, "action_decoder.", plan, obs[:, :-1])
    ad_loss = logistic_loss(lp, ls, mm, acts[:, :-1])
    logs["action_loss"] = ad_loss.item()
    if spec.finetune_action_decoder and optimize:
        g = _grads(ad_loss, P, group_names(P, "action_decoder."), retain=False)
        grads.update(g)
        opts["action_decoder"].step(P, g)
    # get_rl_batch :68-89
    s, nx = torch.cat([obs[:, 0], goal], -1), torch.cat([obs[:, -1], goal], -1)
    r = batch["goal_reached"].long().unsqueeze(-1)
    nz = {k: v.to(dt) for k, v in noise.items() if k != "eps_pr"}
    if optimize:
        grads.update(ac_update(P, opts, spec, s, nx, plan, r, r.clone(), nz, epoch, logs))
    else:
        keep = {k: v.detach().clone() for k, v in P.items()}
        frozen = _FrozenOpts()
        ac_update(P, {k: frozen for k in ("alpha", "alpha_prime", "actor", "q1", "q2")}, _no_polyak(spec), s, nx, plan, r,
                  r.clone(), nz, epoch, logs)
        assert all(torch.equal(keep[k], v) for k, v in P.items())
    return logs, plan, grads


class _FrozenOpts:
    def step(self, P, grads):
        pass


def _no_polyak(spec):
    s = Spec(**{k: v for k, v in spec.__dict__.items()})
    s.tau = 0.0
    return s


def playlmp_step(P, opt, batch, noise, kl_beta=1e-3, kl_alpha=0.8, dropout_p=0.0, step=True):
    """PlayLMP.training_step + its one Adam (play_lmp_d4rl.py:108-144,194-204,235-241).  noise: `dropout` (the plan
    recognition's keep masks, train mode), `eps_plan` (B,A), `u_plan` (B,A) U(0,1).  Returns (logs, gradients, plan)."""
    logs = {}
    dt = next(iter(P.values())).dtype
    obs, acts = batch["observations"].to(dt), batch["actions"].to(dt)[:, :-1]
    mu_p, std_p = policy(P, "plan_proposal.policy.", torch.cat([obs[:, 0], obs[:, -1, :GOAL_DIM]], -1))
    mu_q, std_q = O.plan_recognition(P, "plan_recognition.", obs, dropout=(dropout_p, noise["dropout"]) if dropout_p > 0 else None)
    kl = O.balanced_kl(mu_q, std_q, mu_p, std_p, kl_alpha)
    logs["kl_loss"], logs["kl_loss_scaled"] = kl.item(), (kl * kl_beta).item()
    plan = torch.tanh(mu_q + noise["eps_plan"].to(dt) * std_q)
    action_loss = logistic_loss(*action_decoder_fwd(P, "action_decoder.", plan, obs[:, :-1]), acts)
    logs["action_loss"] = action_loss.item()
    with torch.no_grad():
        rplan = noise["u_plan"].to(dt) * 2.0 - 1.0
        logs["random_plan_action_loss"] = logistic_loss(*action_decoder_fwd(P, "action_decoder.", rplan, obs[:, :-1]), acts).item()
    total = kl * kl_beta + action_loss
    logs["total_loss"] = total.item()
    g = _grads(total, P, [n for n, t in P.items() if t.requires_grad], retain=False)
    if step:
        opt.step(P, g)
    return logs, g, plan.detach()
