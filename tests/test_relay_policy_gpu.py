"""The relay-imitation rollout on the GPU: the fixture rollout_ril (tools/gen_ril_rollout_golden.py, the unmodified reference)
end to end - images in - through the module's rollout surface, through RelayPolicy.step and through step_embeddings; the
per-row schedule against the same rows run alone; the two routes of a chain against each other and against the fp64
restatement; sub-goal overrides; rollout_episodes on four fake image environments whose episodes end at different steps."""
import types

import numpy as np
import pytest
import torch

from tests import ril_util as U
from tests import rows_policy_ref as RP
from tests.golden_util import Golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-4  # the project's fp32 parity bar


def _module(cfg, params=None):
    from tacorl_amd.modules.relay_imitation_learning.relay_imitation_learning import RelayImitationLearning

    mod = RelayImitationLearning(device=DEV, **cfg)
    if params is not None:
        mod.load_state_dict(params)
    mod.eval()
    return mod


@pytest.fixture(scope="module")
def golden():
    g = Golden("rollout_ril")
    c = g.cfg
    batches = [U.make_ril_batch(c["seed"] * 100 + t, c["B"], g.cams) for t in range(c["steps"])]
    return types.SimpleNamespace(g=g, z=g.z, c=c, mod=_module(U.cfg_of_golden(g), g.params()), obs=[b["obs"] for b in batches],
                                 goal=batches[0]["high_level_goal"])


@pytest.fixture(scope="module")
def small():
    """A 2 x 72 module on the golden's two cameras in opposite orders, parameters from its own initialisation."""
    torch.manual_seed(11)
    return _module(U.ril_cfg(low=["rgb_static", "rgb_gripper"], high=["rgb_gripper", "rgb_static"], num_layers=2, hidden_dim=72))


def _embs(R, T, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda: {c: torch.randn(R, 32, generator=g) for c in ("rgb_static", "rgb_gripper")}  # noqa: E731
    return [mk() for _ in range(T)], [mk() for _ in range(T)]


# ------------------------------------------------------------------------------------------ the fixture
def test_golden_through_the_module_surface(golden):
    z, c, mod = golden.z, golden.c, golden.mod
    pe = mod.perceptual_encoder
    assert mod.high_level_policy.action_dim == 32 and mod.high_level_policy.discrete_gripper is False
    assert mod.low_level_policy.action_dim == 7 and mod.low_level_policy.discrete_gripper is True
    with torch.no_grad():
        # the reference manager's own call sequence (evaluation/rollout_manager.py:481-510)
        emb = pe.get_state_from_observation(observation=golden.obs[0], modalities=mod.all_modalities, cat_output=False)
        assert sorted(emb) == sorted(golden.g.cams)
        for k in emb:
            assert U.rel_err(emb[k].cpu(), z[f"emb/{k}"][0]) < RTOL, k
        state_h = torch.cat([emb[k] for k in mod.high_level_policy_modalities], dim=-1)
        goal_in = pe.get_state_from_observation(observation=golden.goal, modalities=mod.high_level_policy_modalities)
        assert U.rel_err(goal_in.cpu(), z["goal_in"]) < RTOL
        goal_out = mod.goal_encoder(goal_in)
        assert U.rel_err(goal_out.cpu(), z["goal_out"]) < RTOL
        high_obs = torch.cat([state_h, goal_out], dim=-1)
        assert U.rel_err(mod.high_level_policy.get_dist(high_obs).normal_mean.cpu(), z["high_mean"]) < RTOL
        sub, lp = mod.high_level_policy.get_actions(high_obs, deterministic=True)
        assert sub.shape == (3, 32) and float(lp.abs().max()) == 0.0 and U.rel_err(sub.cpu(), z["subgoal"]) < RTOL
        for t in range(c["steps"]):
            state_l = pe.get_state_from_observation(observation=golden.obs[t], modalities=mod.low_level_policy_modalities)
            low_obs = torch.cat([state_l, sub], dim=-1)
            assert U.rel_err(mod.low_level_policy.get_dist(low_obs).normal_mean.cpu(), z["low_mean"][t]) < RTOL
            a, _ = mod.low_level_policy.get_actions(low_obs, deterministic=True)
            a = a.cpu()
            assert a.shape == (3, 7) and U.rel_err(a[:, :-1], z["actions"][t][:, :-1]) < RTOL, t
            assert np.array_equal(a[:, -1].numpy(), z["actions"][t][:, -1]), t


def test_golden_through_the_policy(golden):
    from tacorl_amd.evaluation.vec_policy import RelayPolicy

    z, c = golden.z, golden.c
    pol = RelayPolicy(golden.mod, n_envs=3, plan_duration=16)
    assert pol.rows_route(3) == "rows"
    for way in ("step", "step_embeddings"):
        pol.reset()
        for t in range(c["steps"]):
            if way == "step":
                a = pol.step(golden.obs[t], golden.goal)
            else:
                a = pol.step_embeddings({k: torch.from_numpy(z[f"emb/{k}"][t]) for k in golden.g.cams},
                                        {k: torch.from_numpy(z[f"goal_emb/{k}"]) for k in golden.g.cams})
            a = a.cpu()
            if t == 0:
                assert U.rel_err(pol.subgoal.cpu(), z["subgoal"]) < RTOL, way
            assert a.shape == (3, 7) and U.rel_err(a[:, :-1], z["actions"][t][:, :-1]) < RTOL, (way, t)
            assert np.array_equal(a[:, -1].numpy(), z["actions"][t][:, -1]), (way, t)
        assert pol.clock.age == [c["steps"]] * 3


# ------------------------------------------------------------------------------------------ schedule
def test_schedule_rows_equal_the_same_row_alone(small):
    """R = 5, plan_duration 3, eight steps, staggered resets: a step is copies and the rows kernel, so every row's actions and
    sub-goals are bit-identical to that row run alone through an R = 1 policy."""
    from tacorl_amd.evaluation.vec_policy import RelayPolicy

    R, T = 5, 8
    obs, goal = _embs(R, T, seed=21)
    resets = {2: [1], 5: [0, 3]}

    def run(rows):
        pol = RelayPolicy(small, n_envs=len(rows), plan_duration=3)
        pol.reset()
        acts, subs, due = [], [], []
        for t in range(T):
            hit = [rows.index(r) for r in resets.get(t, []) if r in rows]
            if hit:
                pol.reset(hit)
            due.append([rows[i] for i in pol.clock.due()])
            take = lambda d: {k: v[rows] for k, v in d.items()}  # noqa: E731
            acts.append(pol.step_embeddings(take(obs[t]), take(goal[t])).clone().cpu())
            subs.append(pol.subgoal.clone().cpu())
        return acts, subs, due

    full, subs, due = run(list(range(R)))
    assert due == [[0, 1, 2, 3, 4], [], [1], [0, 2, 3, 4], [], [0, 1, 3], [2, 4], []]
    assert all(a.shape == (R, 7) and bool(torch.isfinite(a).all()) and bool((a[:, -1].abs() == 1).all()) for a in full)
    for r in range(R):
        alone, sub1, _ = run([r])
        for t in range(T):
            assert torch.equal(alone[t][0], full[t][r]) and torch.equal(sub1[t][0], subs[t][r]), (r, t)
    assert not torch.equal(full[2][1], full[2][0])


def test_subgoals_override_with_nan_rows(small):
    from tacorl_amd.evaluation.vec_policy import RelayPolicy

    R = 3
    obs, goal = _embs(R, 2, seed=22)
    pol = RelayPolicy(small, n_envs=R, plan_duration=4)
    pol.reset()
    plain = pol.step_embeddings(obs[0], goal[0]).clone()
    own = pol.subgoal.clone()
    given = torch.full((R, 32), float("nan"))
    given[1] = torch.linspace(-0.9, 0.9, 32)
    for sg in (given, given.to(DEV)):  # a host tensor (the row is not computed) and a device tensor (it is, and dropped)
        pol.reset()
        a = pol.step_embeddings(obs[0], goal[0], subgoals=sg)
        assert torch.equal(pol.subgoal[1].cpu(), given[1]) and torch.equal(pol.subgoal[[0, 2]], own[[0, 2]])
        assert torch.equal(a[[0, 2]], plain[[0, 2]]) and not torch.equal(a[1], plain[1])
        b = pol.step_embeddings(obs[1], goal[1], subgoals=torch.zeros(R, 32)).clone()  # not due: ignored
        assert torch.equal(pol.subgoal[1].cpu(), given[1]) and bool(torch.isfinite(b).all())
    all_given = torch.linspace(-1, 1, R * 32).reshape(R, 32)
    pol.reset()
    pol.step_embeddings(obs[0], goal[0], subgoals=all_given)
    assert torch.equal(pol.subgoal.cpu(), all_given)


# ------------------------------------------------------------------------------------------ routing
class _CallLog:
    """The entry points the policy's chains call, in order (a wrapper around `call` where the chains find it)."""

    def __init__(self, monkeypatch):
        import tacorl_amd.modules.inference as I
        import tacorl_amd.ops as O

        self.names = []
        for M in (I, O):
            real = M.call
            monkeypatch.setattr(M, "call", lambda name, *a, real=real: (self.names.append(name), real(name, *a))[1])


def test_chains_route_by_row_count(small, monkeypatch):
    """Up to RelayPolicy.ROWS_KERNEL_MAX_R rows each chain is ONE tacorl_rows_mlp_fwd call; above it, ops.mlp_fwd per chain, the
    sampling kernel per policy head and one column copy for the goal embedding (profiles/ril_rollout.md).  Asserted from the
    entry points a first step (every row re-plans) called."""
    from tacorl_amd.evaluation.vec_policy import RelayPolicy

    M = RelayPolicy.ROWS_KERNEL_MAX_R
    assert 1 <= M <= 64
    log = _CallLog(monkeypatch)
    # the class's threshold (no policy has more than 64 rows: above it only the rule can be asked), then a threshold of 16 set
    # on the instances, at the threshold and one above
    cases = [(1, "rows", None), (M, "rows", None)] + ([(M + 1, "composed", None)] if M < 64 else []) + \
        [(16, "rows", 16), (17, "composed", 16), (64, "composed", 16)]
    assert RelayPolicy(small, n_envs=1).rows_route(M + 1) == "composed"
    for R, route, limit in cases:
        pol = RelayPolicy(small, n_envs=R, plan_duration=2)
        if limit is not None:
            pol.ROWS_KERNEL_MAX_R = limit
        assert pol.rows_route(R) == route
        obs, goal = _embs(R, 2, seed=R)
        pol.reset()
        del log.names[:]
        a = pol.step_embeddings(obs[0], goal[0])
        assert a.shape == (R, 7) and bool(torch.isfinite(a).all())
        count = {k: log.names.count(k) for k in ("tacorl_rows_mlp_fwd", "tacorl_mlp_fwd", "tacorl_tanh_normal_sample", "tacorl_copy_cols")}
        want = (3, 0, 0, 0) if route == "rows" else (0, 3, 2, 1)
        assert tuple(count.values()) == want, (R, log.names)
        del log.names[:]
        pol.step_embeddings(obs[1], goal[1])  # nobody is due: the low-level chain alone
        assert log.names.count("tacorl_rows_mlp_fwd") == (1 if route == "rows" else 0), (R, log.names)
        assert log.names.count("tacorl_mlp_fwd") == (0 if route == "rows" else 1), (R, log.names)


def _problem_of(mod, key):
    """The low- or high-level policy of a module as a tests/rows_policy_ref.py problem (weights as they lie in the module)."""
    sd = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    pre = f"{key}_level_policy.policy."
    L = sum(1 for k in sd if k.startswith(pre + "fc_layers.") and k.endswith(".weight"))
    parts = ["fc_mean", "fc_log_std"] + (["gripper_action"] if pre + "gripper_action.weight" in sd else [])
    W = [sd[f"{pre}fc_layers.{i}.weight"] for i in range(L)] + [torch.cat([sd[f"{pre}{n}.weight"] for n in parts])]
    b = [sd[f"{pre}fc_layers.{i}.bias"] for i in range(L)] + [torch.cat([sd[f"{pre}{n}.bias"] for n in parts])]
    Ac = sd[pre + "fc_mean.bias"].numel()
    return dict(L=L, W=W, b=b, Ac=Ac, dg=len(parts) == 3, acts=[RP.ACT_SILU] * L + [RP.ACT_NONE])


@pytest.mark.parametrize("R", [3, 17])
def test_composed_route_against_the_rows_route(golden, R):
    """The low-level chain of the configured 4 x 1024 module through both routes on one input: every hidden layer of either
    route inside the restatement's bound on that route's own input of the layer, either route's action inside the epilogue's
    bound on its own last hidden layer, the gripper column equal in every row (the inputs are the fixture's rows, whose
    decisions the gap condition keeps 100 x the parity tolerance from a tie)."""
    from tacorl_amd import ops
    from tacorl_amd.evaluation.vec_policy import RelayPolicy

    z, mod = golden.z, golden.mod
    pol = RelayPolicy(mod, n_envs=R, plan_duration=16)
    rep = lambda a: torch.from_numpy(np.concatenate([a] * (R // 3 + 1))[:R].copy())  # noqa: E731
    obs = {k: rep(z[f"emb/{k}"][0]).to(DEV) for k in golden.g.cams}
    pol.subgoal.copy_(rep(z["subgoal"]))
    p = _problem_of(mod, "low")
    chain = pol.low
    dims, n_hid = chain.dims, len(chain.dims) - 2
    a_rows = pol.decode(obs, route="rows").clone().cpu()
    x = pol.lin[:, :pol.E].clone().cpu()
    hid_rows = [chain.hidden(R, l).clone().cpu() for l in range(n_hid)]
    a_comp = pol.decode(obs, route="composed").clone().cpu()
    yoff = ops.mlp_act_layout(R, dims, chain.acts)[1]
    hid_comp = [chain.act[yoff[l]: yoff[l] + R * dims[l + 1]].view(R, dims[l + 1]).clone().cpu() for l in range(n_hid)]
    for name, hid, a in (("rows", hid_rows, a_rows), ("composed", hid_comp, a_comp)):
        h = x
        for l in range(n_hid):
            ref, bnd = RP.layer_ref(p, l, h)
            err = (hid[l].double() - ref).abs()
            assert bool((err <= bnd).all()), (name, l, (err / bnd).max().item())
            h = hid[l]
        ref, bnd, _, _ = RP.action_ref(p, h)
        err = (a[:, :-1].double() - ref[:, :-1]).abs()
        print(f"R {R} {name}: action worst |err| / bound = {(err / bnd).max().item():.3g}")
        assert bool((err <= bnd).all()), (name, (err / bnd).max().item())
        assert torch.equal(a[:, -1].double(), ref[:, -1]), name
    assert torch.equal(a_rows[:, -1], a_comp[:, -1])
    assert U.rel_err(a_comp[:, :-1], a_rows[:, :-1]) < RTOL
    want = rep(z["actions"][0])
    assert torch.equal(a_rows[:, -1], want[:, -1]) and U.rel_err(a_rows[:, :-1], want[:, :-1]) < RTOL


# ------------------------------------------------------------------------------------------ episodes
class ImageEnv:
    """A gym-API stand-in with image observations: frames drawn from (seed, step), a fixed goal, reward = the action's sum."""

    HW = {"rgb_static": (84, 84), "rgb_gripper": (64, 64)}

    def __init__(self, seed, length):
        self.seed, self.length, self._max_episode_steps, self.t = seed, length, 100, 0
        self.goal = self._frame(10_000)

    def _frame(self, t):
        g = torch.Generator().manual_seed(1000 * self.seed + t)
        return {c: (torch.rand(3, h, w, generator=g) * 2 - 1).numpy() for c, (h, w) in self.HW.items()}

    def reset(self):
        self.t = 0
        return self._frame(0)

    def step(self, action):
        self.t += 1
        return self._frame(self.t), float(np.asarray(action, dtype=np.float64).sum()), self.t >= self.length, {"success": self.t % 2 == 0}


def _batch_obs(raw, envs):
    stack = lambda ds: {c: torch.as_tensor(np.stack([d[c] for d in ds])) for c in ImageEnv.HW}  # noqa: E731
    return stack(raw), stack([e.goal for e in envs])


def test_rollout_episodes_four_at_once_equal_four_alone(small):
    from tacorl_amd.evaluation.vec_policy import RelayPolicy, rollout_episodes

    lengths = [3, 6, 6, 8]
    envs = lambda: [ImageEnv(seed=60 + i, length=n) for i, n in enumerate(lengths)]  # noqa: E731
    pol = RelayPolicy(small, n_envs=4, plan_duration=3)
    infos = rollout_episodes(pol, envs(), batch_obs=_batch_obs)
    assert [i["episode_length"] for i in infos] == lengths
    assert all(set(i) == {"episode_length", "episode_return", "success"} for i in infos)
    assert [i["success"] for i in infos] == [n % 2 == 0 for n in lengths]
    for r, env in enumerate(envs()):
        one = rollout_episodes(RelayPolicy(small, n_envs=1, plan_duration=3), [env], batch_obs=_batch_obs)[0]
        assert one["episode_length"] == infos[r]["episode_length"]
        assert one["episode_return"] == infos[r]["episode_return"], (r, one["episode_return"], infos[r]["episode_return"])
    capped = rollout_episodes(pol, envs(), max_steps=2, batch_obs=_batch_obs)
    assert [i["episode_length"] for i in capped] == [2, 2, 2, 2]


# ------------------------------------------------------------------------------------------ refusals
def test_constructor_refusals(small):
    from tacorl_amd.evaluation.vec_policy import RelayPolicy

    with pytest.raises(ValueError):
        RelayPolicy(types.SimpleNamespace(dev=torch.device(DEV)), n_envs=2)  # a module without the two policies
    with pytest.raises(ValueError):
        RelayPolicy(small, n_envs=65)
    with pytest.raises(ValueError):
        RelayPolicy(small, n_envs=0)
    assert RelayPolicy(small, n_envs=64).R == 64
