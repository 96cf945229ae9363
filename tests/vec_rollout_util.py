"""Helpers of tests/test_vec_policy_{cpu,gpu}.py: a deterministic linear fake environment with the gym API, the fp64
restatement of one action-decoder step (ReLU RNN cell per layer, heads, the mixture sampler of seq_ops.hip) with each layer's
a-priori fp32 error bound on its own operands, and the literal per-environment transcription of the reference's rollout
loop the schedule is checked against."""
import numpy as np
import torch

from tests import rows_linear_ref as RL
from tests.action_decoder_util import HEADS, make_params

SEED = 3            # the committed seed of the step_rows-against-act case (tests/test_vec_policy_cpu.py: no case left out)
STEPS, ROWS = 5, 3
LEFT_OUT_CAP = 0.02


# ------------------------------------------------------------------------------------------------ fake environment
class LinearEnv:
    """obs' = A obs + B a; reward = -|obs'[:2] - goal|; done after `length` steps.  Everything is float64 numpy on the host,
    so an episode's return is a function of the action bits alone."""

    def __init__(self, seed, length, state_dim=29, action_dim=8, max_episode_steps=20):
        g = np.random.RandomState(seed)
        self.A = np.eye(state_dim) * 0.9 + g.randn(state_dim, state_dim) * 0.02
        self.B = g.randn(state_dim, action_dim) * 0.1
        self.obs0 = g.randn(state_dim)
        self.target_goal = g.randn(2)
        self.length, self._max_episode_steps = length, max_episode_steps
        self.t, self.obs = 0, None

    def reset(self):
        self.t, self.obs = 0, self.obs0.copy()
        return self.obs.astype(np.float32)

    def step(self, a):
        self.obs = self.A @ self.obs + self.B @ np.asarray(a, dtype=np.float64)
        self.t += 1
        reward = -float(np.abs(self.obs[:2] - self.target_goal).sum())
        done = self.t >= self.length
        return self.obs.astype(np.float32), reward, done, {"success": done and reward > -1.0}


# ------------------------------------------------------------------------------------------------ decoder step in fp64
def decoder_problem(H, P=16, E=32, L=2, seed=SEED, R=ROWS, steps=STEPS, Da=6, K=10):
    """Weights (action_decoder_util.make_params: the reference's names), per-step plans / embeddings / draws."""
    W = make_params(H, P + E, L, seed)
    g = torch.Generator().manual_seed(seed + 1)
    plan = torch.randn(R, P, generator=g).tanh()
    emb = [torch.randn(R, E, generator=g) for _ in range(steps)]
    ra = [torch.rand(R, Da, K, generator=g) for _ in range(steps)]
    rb = [torch.rand(R, Da, generator=g) for _ in range(steps)]
    restart = [[True] * R if t == 0 else [t == 2 and r == 1 for r in range(R)] for t in range(steps)]
    return dict(W=W, plan=plan, emb=emb, ra=ra, rb=rb, restart=restart, H=H, P=P, E=E, L=L, R=R, Da=Da, K=K, steps=steps)


def head_matrix(W):
    return (torch.cat([W[n + ".weight"] for n in HEADS]), torch.cat([W[n + ".bias"] for n in HEADS]))


def decoder_step64(pb, t, h, restart=None, own_h=None):
    """One step in fp64 from the hidden state h [L x (R,H)], taken as exact data (rows flagged in `restart`, default
    pb['restart'][t], start from zeros; own_h: a path's own fp32 layer outputs, fed to the next layer and to the heads in
    place of this function's - the operands that path's next layer really had), with the a-priori bound
    of an fp32 evaluation of EACH LAYER on its own operands, gamma_{K+4} (|b| + sum |w||x|) (tests/rows_linear_ref.py).
    The bound is per layer, not carried on: through |W| the worst case grows by the matrices' absolute row sums - about 22 per
    layer at H = 2048, 1.3 in absolute terms at the heads after two layers, more than the scores' gaps - so a path is held
    to each layer's bound on the operands that path itself fed it.
    Returns (heads (R,NH), head_err, actions (R,Da+1), gap (R,Da+1): the distance between the sampler's two best scores - the
    two gripper logits for the last column -, new h [L x (R,H)], h_err [L x (R,H)])."""
    W, d = pb["W"], torch.float64
    flag = torch.tensor(pb["restart"][t] if restart is None else restart)
    x = torch.cat([pb["plan"], pb["emb"][t]], dim=1).to(d)
    nh, nerr = [], []
    for l in range(pb["L"]):
        wi, wh = W[f"rnn.weight_ih_l{l}"].to(d), W[f"rnn.weight_hh_l{l}"].to(d)
        bi, bh = W[f"rnn.bias_ih_l{l}"].to(d), W[f"rnn.bias_hh_l{l}"].to(d)
        hp = h[l].to(d).clone()
        hp[flag] = 0.0
        z = x @ wi.T + bi + hp @ wh.T + bh
        scale = x.abs() @ wi.abs().T + bi.abs() + hp.abs() @ wh.abs().T + bh.abs()
        x = torch.relu(z)
        nh.append(x)
        nerr.append(RL.gamma(wi.shape[1] + wh.shape[1] + 4) * scale)
        x = x if own_h is None else own_h[l].to(d)
    hw, hb = head_matrix(W)
    hw, hb = hw.to(d), hb.to(d)
    heads = x @ hw.T + hb
    head_err = RL.gamma(hw.shape[1] + 4) * (x.abs() @ hw.abs().T + hb.abs())
    Da, K, R = pb["Da"], pb["K"], pb["R"]
    mean, lsc, lg = (heads[:, i * Da * K: (i + 1) * Da * K].view(R, Da, K) for i in range(3))
    r1, r2 = 1e-5, 1.0 - 1e-5
    score = lg - torch.log(-torch.log((r1 - r2) * pb["ra"][t].to(d) + r2))
    top = score.topk(2, dim=-1)
    arg = top.indices[..., :1]
    ls = lsc.gather(-1, arg).squeeze(-1).clamp_min(-5.0)
    u = (r1 - r2) * pb["rb"][t].to(d) + r2
    arm = mean.gather(-1, arg).squeeze(-1) + ls.exp() * (torch.log(u) - torch.log(1.0 - u))
    g0, g1 = heads[:, 3 * Da * K], heads[:, 3 * Da * K + 1]
    grip = torch.where(g1 > g0, 1.0, -1.0).to(d)
    actions = torch.cat([arm, grip.unsqueeze(1)], dim=1)
    gap = torch.cat([top.values[..., 0] - top.values[..., 1], (g1 - g0).abs().unsqueeze(1)], dim=1)
    return heads, head_err, actions, gap, nh, nerr


def cross_path_bounds(pb, t, ref_a, ref_b, prev_a, prev_b, new_a, new_b):
    """Bounds on the difference of two fp32 paths at step t, layer by layer, from nothing but what the layer was FED:
        |h_a[l] - h_b[l]| <= E_a[l] + E_b[l] + |W_ih| |x_a - x_b| + |W_hh| |hprev_a - hprev_b|
    (each path within its own a-priori bound E of the fp64 image of its operands - decoder_step64's ref_a / ref_b - and the
    two fp64 images apart by at most the weights' absolute values times the operands' difference; ReLU is 1-Lipschitz).
    x is the same [plan | emb] for layer 0 and the paths' own outputs of the layer below after that; hprev are the paths'
    hidden states before the step WITH THE RESTARTED ROWS ZEROED, as the step is specified - a path that does not clear a
    row gets no allowance for it.  The operands' differences are themselves outputs that this bound held to account one layer
    or one step earlier; at step 0 they are zero.  The heads likewise: E_a + E_b + |W_head| |top_a - top_b|.
    Returns ([L x (R,H)], (R,NH))."""
    W, d = pb["W"], torch.float64
    flag = torch.tensor(pb["restart"][t])
    dx = torch.zeros(pb["R"], pb["P"] + pb["E"], dtype=d)
    out = []
    for l in range(pb["L"]):
        dp = (prev_a[l].to(d) - prev_b[l].to(d)).abs()
        dp[flag] = 0.0
        b = (ref_a[5][l] + ref_b[5][l] + dx @ W[f"rnn.weight_ih_l{l}"].to(d).abs().T + dp @ W[f"rnn.weight_hh_l{l}"].to(d).abs().T)
        out.append(b)
        dx = (new_a[l].to(d) - new_b[l].to(d)).abs()
    hw, _ = head_matrix(W)
    return out, ref_a[1] + ref_b[1] + dx @ hw.to(d).abs().T


def decoder_step32(pb, t, h, clear=True, split=1):
    """An fp32 path in plain torch: the step with every product summed in `split` pieces (another summation order per value of
    split).  clear=False leaves the restarted rows' hidden state as it is - the fault the cross-path bounds must catch.
    Returns (heads (R,NH), new h [L x (R,H)]) in fp32."""
    W, f = pb["W"], torch.float32
    flag = torch.tensor(pb["restart"][t])

    def mm(x, w):
        n = x.shape[1]
        cuts = [n * i // split for i in range(split + 1)]
        acc = torch.zeros(x.shape[0], w.shape[0], dtype=f)
        for a_, b_ in zip(cuts[:-1], cuts[1:]):
            if b_ > a_:
                acc = acc + x[:, a_:b_] @ w[:, a_:b_].T
        return acc

    x = torch.cat([pb["plan"], pb["emb"][t]], dim=1).to(f)
    nh = []
    for l in range(pb["L"]):
        hp = h[l].to(f).clone()
        if clear:
            hp[flag] = 0.0
        z = mm(x, W[f"rnn.weight_ih_l{l}"]) + W[f"rnn.bias_ih_l{l}"] + mm(hp, W[f"rnn.weight_hh_l{l}"]) + W[f"rnn.bias_hh_l{l}"]
        x = torch.relu(z)
        nh.append(x)
    hw, hb = head_matrix(W)
    return mm(x, hw) + hb, nh


def deciding_bound(pb, head_bound):
    """(R, Da+1): per sampled dimension the largest entry of a heads bound (R,NH) among the logits that decide it (the K
    mixture logits of the dimension; the two gripper logits)."""
    R, Da, K = pb["R"], pb["Da"], pb["K"]
    lg = head_bound[:, 2 * Da * K: 3 * Da * K].view(R, Da, K).max(dim=-1).values
    gr = head_bound[:, 3 * Da * K: 3 * Da * K + 2].max(dim=-1).values
    return torch.cat([lg, gr.unsqueeze(1)], dim=1)


def decoder_rollout64(pb):
    """All steps in fp64: lists of heads, head_err, actions, gap and `left_out` (R, Da+1) bool per step - the cases a comparison
    of two fp32 paths may leave out: the two best scores closer than twice the heads' bound, the sum of both paths' (here
    equal) a-priori bounds."""
    R, H = pb["R"], pb["H"]
    h = [torch.zeros(R, H, dtype=torch.float64) for _ in range(pb["L"])]
    out = dict(heads=[], head_err=[], actions=[], gap=[], left_out=[])
    for t in range(pb["steps"]):
        heads, he, actions, gap, h, _ = decoder_step64(pb, t, h)
        left = gap < 2 * deciding_bound(pb, 2 * he)
        for k, v in (("heads", heads), ("head_err", he), ("actions", actions), ("gap", gap), ("left_out", left)):
            out[k].append(v)
    out["hidden"] = h
    return out


# ------------------------------------------------------------------------------------------------ the reference's loop
def reference_loop(plan_fn, decoder_fn, observations, goals, row, episode_lengths, plan_duration, hidden0, plans=None):
    """evaluation/rollout_manager_d4rl.py:137-157 for ONE environment (row `row` of the per-step inputs), episode after
    episode: `while not done: plan; clear_hidden_state(); for _ in range(plan_duration): act; step; if done: break`.
    The environment is the recorded inputs: global step t feeds observations[t][row]; an episode is done after its length.
    Returns (actions per global step, the global steps at which a plan was made)."""
    t, actions, planned = 0, [], []
    for length in episode_lengths:
        step, done = 0, False
        while not done:
            obs, goal = observations[t][row: row + 1], goals[t][row: row + 1]
            given = plans is not None and t in plans and not bool(torch.isnan(plans[t][row]).any())
            latent_plan = plans[t][row: row + 1] if given else plan_fn(obs, goal, [row], t)
            planned.append(t)
            hidden = hidden0.clone()  # action_decoder.clear_hidden_state()
            for _ in range(plan_duration):
                a, hidden = decoder_fn(latent_plan, observations[t][row: row + 1], hidden, t)
                actions.append(a[0])
                t += 1
                step += 1
                done = step >= length
                if done:
                    break
    return actions, planned
