"""RelayPolicy's schedule without a GPU: relay_policy_restatement against a literal per-environment transcription of the
reference manager's two nested loops (evaluation/rollout_manager.py:480-532), and the fixture rollout_ril
(tools/gen_ril_rollout_golden.py, the unmodified reference) reproduced by plain-torch fp32 policies built from its seed."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import ril_util as U
from tests.golden_util import Golden

CAMS = ["rgb_static", "rgb_gripper"]
GAP = 1e-2  # tools/gen_ril_rollout_golden.py: 100 x the parity tolerance


# ---------------------------------------------------------------------------------- schedule
def _high(obs, goal):
    """Row-wise and elementwise (so that a row alone and the row in a batch agree to the bit): (n, 32)."""
    return torch.tanh(obs["rgb_gripper"] - 0.5 * obs["rgb_static"] + goal["rgb_static"] * goal["rgb_gripper"])


def _low(obs, sub):
    a = torch.tanh(obs["rgb_static"][:, :6] * sub[:, :6] + obs["rgb_gripper"][:, 6:12])
    grip = torch.where(sub[:, 7] > obs["rgb_static"][:, 7], 1.0, -1.0)
    return torch.cat([a, grip.unsqueeze(1)], dim=1)


def test_restatement_against_the_managers_two_loops():
    from tacorl_amd.evaluation.vec_policy import relay_policy_restatement

    R, D, T = 4, 3, 12
    g = torch.Generator().manual_seed(3)
    obs = [{c: torch.randn(R, 32, generator=g) for c in CAMS} for _ in range(T)]
    goal = [{c: torch.randn(R, 32, generator=g) for c in CAMS} for _ in range(T)]
    resets = {4: [1], 5: [2, 3], 7: [1], 11: [0]}  # an environment's episode ends: its next step starts a new one
    calls = []

    def high_fn(o, gl, rows, t):
        calls.append((t, list(rows)))
        return _high(o, gl)

    got = relay_policy_restatement(high_fn, lambda o, s, t: _low(o, s), obs, goal, R, D, resets=resets)
    assert all(len(rows) == 1 for _, rows in calls)  # one row at a time: only the rows that are due
    # the manager, one environment at a time: an episode from each reset to the next
    for r in range(R):
        starts = [0] + [t for t in sorted(resets) if r in resets[t]] + [T]
        planned = []
        for t0, t1 in zip(starts[:-1], starts[1:]):
            step = t0
            while step < t1:                                                   # while not done and step < max_episode_steps
                row = lambda d: {c: v[r: r + 1] for c, v in d.items()}         # noqa: E731
                latent_subgoal = _high(row(obs[step]), row(goal[step]))        # :481-499
                planned.append(step)
                for _ in range(D):                                             # :501
                    action = _low(row(obs[step]), latent_subgoal)              # :502-510
                    assert torch.equal(action[0], got["actions"][step][r]), (r, step)
                    assert torch.equal(latent_subgoal[0], got["subgoal"][step][r]), (r, step)
                    step += 1
                    if step >= t1:                                             # :531
                        break
        assert planned == [t for t in range(T) if r in got["replanned"][t]], (r, planned)
    assert got["replanned"][0] == [0, 1, 2, 3] and got["replanned"][3] == [0, 1, 2, 3] and got["replanned"][4] == [1]
    assert got["replanned"][5] == [2, 3] and got["replanned"][6] == [0] and got["replanned"][1] == []


def test_restatement_subgoals_override_the_high_level_policy():
    from tacorl_amd.evaluation.vec_policy import relay_policy_restatement

    R, D, T = 3, 2, 4
    g = torch.Generator().manual_seed(4)
    obs = [{c: torch.randn(R, 32, generator=g) for c in CAMS} for _ in range(T)]
    goal = [{c: torch.randn(R, 32, generator=g) for c in CAMS} for _ in range(T)]
    given = torch.full((R, 32), float("nan"))
    given[1] = torch.linspace(-1, 1, 32)
    asked = []
    high_fn = lambda o, gl, rows, t: (asked.append((t, rows[0])), _high(o, gl))[1]  # noqa: E731
    got = relay_policy_restatement(high_fn, lambda o, s, t: _low(o, s), obs, goal, R, D, subgoals={0: given, 1: given})
    assert (0, 1) not in asked and (0, 0) in asked and (2, 1) in asked  # step 1 is not due: its sub-goals are ignored
    assert torch.equal(got["subgoal"][1][1], given[1]) and torch.equal(got["subgoal"][0][0], _high(obs[0], goal[0])[0])
    assert torch.equal(got["subgoal"][2][1], _high(obs[2], goal[2])[1])


# ---------------------------------------------------------------------------------- the fixture
def torch_policies(P, high_cams, low_cams):
    """(goal encoder, high-level policy, low-level policy) as plain fp32 torch functions of the reference's parameters."""
    def mlp(x, pre, n):
        for i in range(n):
            x = F.silu(x @ P[f"{pre}fc_layers.{i}.weight"].T + P[f"{pre}fc_layers.{i}.bias"])
        return x

    n_h = sum(1 for k in P if k.startswith("high_level_policy.policy.fc_layers.") and k.endswith(".weight"))
    n_l = sum(1 for k in P if k.startswith("low_level_policy.policy.fc_layers.") and k.endswith(".weight"))
    lin = lambda x, name: x @ P[name + ".weight"].T + P[name + ".bias"]  # noqa: E731

    def genc(x):
        return torch.tanh(lin(F.relu(lin(F.relu(lin(x, "goal_encoder.mlp.0")), "goal_encoder.mlp.2")), "goal_encoder.mlp.4"))

    def high(obs, goal, rows=None, t=None, want_mean=False):
        s = torch.cat([obs[c] for c in high_cams] + [genc(torch.cat([goal[c] for c in high_cams], dim=-1))], dim=-1)
        mean = lin(mlp(s, "high_level_policy.policy.", n_h), "high_level_policy.policy.fc_mean").clamp(-9, 9)
        return mean if want_mean else torch.tanh(mean)

    def low(obs, sub, t=None, want_head=False):
        h = mlp(torch.cat([obs[c] for c in low_cams] + [sub], dim=-1), "low_level_policy.policy.", n_l)
        mean = lin(h, "low_level_policy.policy.fc_mean").clamp(-9, 9)
        lg = lin(h, "low_level_policy.policy.gripper_action")
        if want_head:
            return mean, lg
        return torch.cat([torch.tanh(mean), (torch.argmax(lg, dim=-1, keepdim=True) * 2.0 - 1)], dim=-1)

    return genc, high, low


def test_fixture_meets_the_gap_condition():
    z = Golden("rollout_ril").z
    lg = z["low_logits"]
    assert lg.shape == (3, 3, 2) and z["actions"].shape == (3, 3, 7)
    gap, scale = np.abs(lg[..., 1] - lg[..., 0]), np.maximum(np.abs(lg[..., 0]), np.abs(lg[..., 1]))
    assert np.all(gap >= GAP * scale), (gap / scale).min()
    assert np.array_equal(z["actions"][..., -1], np.where(lg[..., 1] > lg[..., 0], 1.0, -1.0))


def test_fixture_is_reproduced_by_plain_torch_policies():
    from tacorl_amd.evaluation.vec_policy import relay_policy_restatement

    g = Golden("rollout_ril")
    z, c = g.z, g.cfg
    assert c["low"] == ["rgb_static", "rgb_gripper"] and c["high"] == ["rgb_gripper", "rgb_static"] and c["seed"] >= 52
    assert g.cams == {"rgb_static": (84, 84), "rgb_gripper": (64, 64)}
    P = g.params()
    genc, high, low = torch_policies(P, c["high"], c["low"])
    T = c["steps"]
    obs = [{k: torch.from_numpy(z[f"emb/{k}"][t]) for k in g.cams} for t in range(T)]
    goal = {k: torch.from_numpy(z[f"goal_emb/{k}"]) for k in g.cams}
    # the recorded goal-encoder input is the goal embeddings in the high-level policy's order
    assert np.array_equal(z["goal_in"], np.concatenate([z[f"goal_emb/{k}"] for k in c["high"]], axis=-1))
    assert U.rel_err(genc(torch.from_numpy(z["goal_in"])), z["goal_out"]) < 1e-4
    assert U.rel_err(high(obs[0], goal, want_mean=True), z["high_mean"]) < 1e-4
    got = relay_policy_restatement(high, low, obs, [goal] * T, c["B"], 16)
    assert got["replanned"] == [[0, 1, 2]] + [[]] * (T - 1)
    sub = torch.from_numpy(z["subgoal"])
    for t in range(T):
        assert U.rel_err(got["subgoal"][t], z["subgoal"]) < 1e-4
        mean, lg = low(obs[t], sub, want_head=True)
        assert U.rel_err(mean, z["low_mean"][t]) < 1e-4 and U.rel_err(lg, z["low_logits"][t]) < 1e-4
        a = got["actions"][t]
        assert a.shape == (3, 7) and U.rel_err(a[:, :-1], z["actions"][t][:, :-1]) < 1e-4, t
        assert np.array_equal(a[:, -1].numpy(), z["actions"][t][:, -1]), t
