"""Host-side pieces of the rollout evaluation that need no GPU: rl_policy_restatement against a per-environment loop written
from the reference manager's lines, rollout_episodes' reset_infos / successful_tasks / actions_out with a policy stand-in,
the fake environments' determinism, and the IncreaseHorizon callbacks on a TransitionIndex."""
import numpy as np
import pytest
import torch

from tests import rollout_envs as E


# ------------------------------------------------------------------------------------------ RLPolicy's restatement
def _nets(seed, S=6, G=2, A=3):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(A, S + G, generator=g, dtype=torch.float64) * 0.3
    Q = torch.randn(S + G + A, generator=g, dtype=torch.float64)

    def actor(obs, goal):
        # (products summed per row, not a GEMM: a row's result must not depend on how many rows go with it)
        return torch.tanh((torch.cat([obs, goal], dim=-1).unsqueeze(1) * W).sum(dim=-1))

    def cem(obs, goal, mean, eps):
        """One refit per row towards the best of the row's own population: any function of the row and its draws will do."""
        pop = (mean.unsqueeze(1) + 0.3 * eps).clamp(-1, 1)                                   # (R, N, A)
        x = torch.cat([torch.cat([obs, goal], dim=-1).unsqueeze(1).expand(-1, pop.shape[1], -1), pop], dim=-1)
        return pop[torch.arange(pop.shape[0]), (x * Q).sum(dim=-1).argmax(dim=1)]

    return actor, cem


@pytest.mark.parametrize("use_cem", [False, True])
def test_rl_policy_restatement_against_a_per_environment_loop(use_cem):
    """The reference manager (rollout_manager.py:121-141) runs one environment: per step the deterministic action of the
    actor, refined by CEM under use_cem.  The restatement over R rows gives every row exactly what that loop gives it."""
    from tacorl_amd.evaluation.vec_policy import rl_policy_restatement

    R, T, S, G, A, N = 4, 5, 6, 2, 3, 8
    actor, cem = _nets(1, S, G, A)
    g = torch.Generator().manual_seed(2)
    obs = [torch.randn(R, S, generator=g, dtype=torch.float64) for _ in range(T)]
    goal = [torch.randn(R, G, generator=g, dtype=torch.float64) for _ in range(T)]
    eps = [torch.randn(R, N, A, generator=g, dtype=torch.float64) for _ in range(T)]
    out = rl_policy_restatement(lambda o, gl, t: actor(o, gl), obs, goal, R,
                                cem_fn=(lambda o, gl, m, t: cem(o, gl, m, eps[t])) if use_cem else None)
    assert len(out["actions"]) == T and all(a.shape == (R, A) for a in out["actions"])
    for r in range(R):  # the per-environment loop
        for t in range(T):
            o, gl = obs[t][r: r + 1], goal[t][r: r + 1]
            a = actor(o, gl)
            assert torch.equal(out["initial_mean"][t][r], a[0])
            if use_cem:
                a = cem(o, gl, a, eps[t][r: r + 1])
            assert torch.equal(out["actions"][t][r], a[0]), (r, t)
    assert use_cem == any(not torch.equal(a, m) for a, m in zip(out["actions"], out["initial_mean"]))
    with pytest.raises(ValueError, match="action rows"):
        rl_policy_restatement(lambda o, gl, t: actor(o, gl)[:2], obs, goal, R)


# ------------------------------------------------------------------------------------------ rollout_episodes
class _Policy:
    """A stand-in with the policies' shape: the action is a fixed function of the step number and the row."""

    def __init__(self, R):
        self.R, self.resets, self.seen = R, 0, []

    def reset(self, rows=None):
        self.resets += 1

    def step(self, observation, goal, noise=None):
        self.seen.append((observation, goal, noise))
        t = len(self.seen) - 1
        return torch.tensor([[((t + r) % 3 - 1) / 1.0, ((2 * t + r) % 3 - 1) / 1.0] for r in range(self.R)])


def test_rollout_episodes_reset_infos_and_successful_tasks():
    from tacorl_amd.evaluation.vec_policy import rollout_episodes

    envs = [E.GridImageEnv(seed=3, src_hw=(12, 12), max_episode_steps=7) for _ in range(3)]
    infos_in = [{"task_info": {"start_info": E.state_of_step(100 + 9 * r), "goal_info": E.state_of_step(103 + 9 * r),
                               "tasks": [f"task{r}"]}} for r in range(3)]
    acts = []
    batch_obs = lambda raw, envs: (len(raw), None)  # noqa: E731
    pol = _Policy(3)
    got = rollout_episodes(pol, envs, batch_obs=batch_obs, reset_infos=infos_in, actions_out=acts)
    assert pol.resets == 1 and len(got) == 3
    for r, (info, env) in enumerate(zip(got, envs)):
        assert set(info) == {"episode_length", "episode_return", "success", "successful_tasks"}
        assert info["successful_tasks"] == ([f"task{r}"] if info["success"] else [])
        assert len(acts[r]) == info["episode_length"] <= 7
        # the same episode alone, stepped with the recorded actions
        one = E.GridImageEnv(seed=3, src_hw=(12, 12), max_episode_steps=7)
        one.reset(**infos_in[r])
        ret = 0.0
        for a in acts[r]:
            _, rew, done, last = one.step(a)
            ret += rew
        assert ret == info["episode_return"] and last["success"] == info["success"]
    # defaults: no reset_infos -> reset() without arguments; an environment without successful_tasks -> no such key
    vec = [E.PointVectorEnv(seed=1, length=4, action_dim=2) for _ in range(2)]
    out = rollout_episodes(_Policy(2), vec, batch_obs=batch_obs)
    assert [i["episode_length"] for i in out] == [4, 4] and all(set(i) == {"episode_length", "episode_return", "success"} for i in out)
    with pytest.raises(ValueError, match="reset_infos"):
        rollout_episodes(_Policy(2), vec, batch_obs=batch_obs, reset_infos=[{}])


def test_fake_environments_are_pure_functions_of_their_state():
    a, b = E.GridImageEnv(seed=5, cams=("rgb_static", "rgb_gripper"), src_hw={"rgb_static": (20, 24), "rgb_gripper": (10, 10)}), None
    o1 = a.reset(task_info={"task": "open_drawer", "index": 1})
    b = E.GridImageEnv(seed=9, cams=("rgb_static", "rgb_gripper"), src_hw={"rgb_static": (20, 24), "rgb_gripper": (10, 10)})
    o2 = b.reset(task_info={"task": "open_drawer", "index": 1})
    for part in ("observation", "goal"):
        assert o1[part]["rgb_static"].shape == (20, 24, 3) and o1[part]["rgb_static"].dtype == np.uint8
        assert all(np.array_equal(o1[part][c], o2[part][c]) for c in a.cams)
    assert not np.array_equal(o1["observation"]["rgb_static"], o1["goal"]["rgb_static"])
    assert not np.array_equal(o1["observation"]["rgb_static"][:10, :10], o1["observation"]["rgb_gripper"])
    s1 = a.step(np.array([1.0, -1.0, 0.3]))
    s2 = b.step(np.array([1.0, -1.0, 0.3]))
    assert s1[1:] == s2[1:] and np.array_equal(s1[0]["observation"]["rgb_static"], s2[0]["observation"]["rgb_static"])
    assert hasattr(E.PointVectorEnv(), "target_goal")


# ------------------------------------------------------------------------------------------ IncreaseHorizon
def test_increase_horizon_linear_moves_the_index_as_increase_horizon_does():
    from tacorl_amd import lightning as TL
    from tacorl_amd.data.replay import TransitionIndex
    from tacorl_amd.utils.callbacks.increase_horizon import IncreaseHorizonConstant, IncreaseHorizonLinear

    ep = np.array([[0, 40], [50, 99]])
    kw = dict(initial_horizon=8, horizon_step=4, max_horizon=18)
    index = TransitionIndex(ep, n_frames=100, goal_strategy_prob={"geometric": 0.5, "increasing_horizon": 0.5}, **kw)
    twin = TransitionIndex(ep, n_frames=100, goal_strategy_prob={"geometric": 0.5, "increasing_horizon": 0.5}, **kw)
    fixed = TransitionIndex(ep, n_frames=100, goal_strategy_prob={"geometric": 1.0}, **kw)

    class DM:
        def __init__(self, index):
            self.index = index

        def train_dataloader(self):
            return [torch.zeros(1)] * 2

    class Toy(TL.LightningModuleBase):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))
            self.automatic_optimization = False

        if not hasattr(TL.LightningModuleBase, "device"):
            device = torch.device("cpu")

        @property
        def current_epoch(self):
            return self.trainer.current_epoch

        def configure_optimizers(self):
            return torch.optim.SGD([self.w], lr=0.1)

        def training_step(self, batch, batch_idx):
            return {"loss": 0.0}

    seen = []

    class Probe:
        def on_train_epoch_end(self, trainer, pl_module):
            seen.append((trainer.logged_metrics["train/goal_horizon"], trainer.datamodule.index.current_horizon))

    TL.MiniTrainer(max_epochs=4, callbacks=[IncreaseHorizonLinear(), IncreaseHorizonConstant(), Probe()]).fit(Toy(), datamodule=DM(index))
    want = []
    for epoch in range(4):
        before = twin.current_horizon
        twin.increase_horizon(epoch + 1)
        want.append((float(before), twin.current_horizon))
    assert seen == want and [h for _, h in seen] == [12, 16, 18, 18]
    # a dataset without the increasing_horizon strategy: logged, not moved
    tr = TL.MiniTrainer(max_epochs=2, callbacks=[IncreaseHorizonLinear()])
    tr.fit(Toy(), datamodule=DM(fixed))
    assert fixed.current_horizon == 8 and tr.logged_metrics["train/goal_horizon"] == 8.0
