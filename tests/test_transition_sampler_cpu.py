"""TransitionIndex (tacorl_amd/data/replay.py) against the items the reference's GoalCondReplayBufferDataset returned for
recorded draws (tests/golden/transition_sampler.npz), the distributions of its own draws, the horizon schedule and the
constructor's table validation.  No GPU."""
import numpy as np
import pytest

from tests.transition_util import TransitionGolden, coverage

G = TransitionGolden()
VARIANTS = list(G.variants)


def test_fixture_has_every_variant():
    assert VARIANTS == ["geo_sim", "horizon", "horizon_epoch3", "episode_future", "next_state", "random"]
    assert len(G.ep) == 3 and len({int(e - s) for s, e in G.ep}) == 3  # three episodes of unequal length
    assert sorted({len(v) for v in G.nn.values()}) == [0, 1, 2, 3]     # neighbour lists of length 0-3


@pytest.mark.parametrize("variant", VARIANTS)
def test_sample_equals_the_reference_dataset(variant):
    v = G.variants[variant]
    cov = coverage(variant, v, G.ep, G.nn)
    assert cov and all(cov.values()), cov
    ix = G.index(variant)
    assert len(ix) == int(v["len"]) and ix.current_horizon == int(v["horizon"])
    d = G.draws(variant, ix)
    assert np.array_equal(d["strategy"], v["strategy"])
    s = ix.sample(d["idx"], d)
    for k in ("step", "next", "goal", "reward", "done"):
        assert np.array_equal(s[k], v[k]), (k, s[k], v[k])
    assert np.array_equal(G.actions[s["step"]], v["actions"])
    assert np.array_equal(ix.sample(None, d)["goal"], v["goal"])  # idx taken from the draws


def test_draw_follows_the_reference_distributions():
    from tacorl_amd.data.replay import S_GEOMETRIC, S_NEXT, S_SIMILAR, TransitionIndex

    # dict order decides the codes' cumulative order: similar first here
    ix = TransitionIndex(G.ep, goal_strategy_prob={"similar_robot_obs": 0.25, "next_state": 0.0, "geometric": 0.75},
                         goal_sampling_prob=0.3, nn_steps_from_step=G.nn)
    n = 200_000
    d = ix.draw(n, np.random.default_rng(0))
    # binomial / geometric standard errors at n = 2e5: share 0.25 -> 9.7e-4, disp mean 1/0.3 (sd 2.79) -> 6.2e-3,
    # item frequency 1/57 -> 2.9e-4; bounds at 5 sigma
    assert abs((d["strategy"] == S_SIMILAR).mean() - 0.25) < 5e-3 and abs((d["strategy"] == S_GEOMETRIC).mean() - 0.75) < 5e-3
    assert not (d["strategy"] == S_NEXT).any()
    assert d["disp"].min() == 1 and abs(d["disp"].mean() - 1 / 0.3) < 3.1e-2
    cnt = np.bincount(d["idx"], minlength=len(ix))
    assert len(cnt) == len(ix) and np.abs(cnt / n - 1 / len(ix)).max() < 1.5e-3
    assert d["u_choice"].min() >= 0.0 and d["u_choice"].max() < 1.0 and abs(d["u_choice"].mean() - 0.5) < 3.3e-3
    assert np.array_equal(ix.strategy_of([0.0, 0.2499, 0.25, 0.9999]), [S_SIMILAR, S_SIMILAR, S_GEOMETRIC, S_GEOMETRIC])
    # the torch form of the draws (the device path's, run here on the CPU): same ranges and shares
    import torch

    t = ix.draw_device(n, "cpu", torch.Generator().manual_seed(0))
    assert t["idx"].dtype == t["strategy"].dtype == t["disp"].dtype == torch.int64 and t["u_choice"].dtype == torch.float64
    assert int(t["idx"].min()) >= 0 and int(t["idx"].max()) == len(ix) - 1 and int(t["disp"].min()) == 1
    assert abs(float((t["strategy"] == S_SIMILAR).double().mean()) - 0.25) < 5e-3
    assert abs(float(t["disp"].double().mean()) - 1 / 0.3) < 3.1e-2
    s = ix.sample(None, {k: v.numpy() for k, v in t.items()})
    assert s["goal"].min() >= 0 and s["goal"].max() < ix.n_frames and s["next"].max() < ix.n_frames


def test_every_strategy_stays_inside_the_dataset_and_its_episode():
    """All six strategies over many draws: ids in range, future goals inside (step, episode end], random goals != step."""
    from tacorl_amd.data.replay import S_EPISODE, S_GEOMETRIC, S_HORIZON, S_RANDOM, STRATEGIES, TransitionIndex

    ix = TransitionIndex(G.ep, goal_strategy_prob={k: 1 / 6 for k in STRATEGIES}, nn_steps_from_step=G.nn, initial_horizon=5)
    d = ix.draw(20_000, np.random.default_rng(1))
    s = ix.sample(None, d)
    end = ix.episode_end(s["step"])
    assert sorted(set(d["strategy"])) == list(range(6))
    assert s["goal"].min() >= 0 and s["goal"].max() < ix.n_frames and (s["next"] <= end).all()
    fut = np.isin(d["strategy"], (S_GEOMETRIC, S_HORIZON, S_EPISODE))
    assert ((s["goal"] > s["step"]) & (s["goal"] <= end))[fut].all()
    hz = d["strategy"] == S_HORIZON
    assert (s["goal"][hz] - s["step"][hz]).max() == 5
    rnd = d["strategy"] == S_RANDOM
    assert (s["goal"][rnd] != s["step"][rnd]).all() and np.isin(s["goal"][rnd], ix.possible_steps).all()
    assert set(s["goal"][rnd]) == set(ix.possible_steps)  # ... and every other item can be reached
    assert np.array_equal(s["reward"], (s["goal"] == s["step"] + 1).astype(np.int64)) and np.array_equal(s["reward"], s["done"])


def test_increase_horizon_saturates():
    from tacorl_amd.data.replay import TransitionIndex

    ix = TransitionIndex(G.ep, goal_strategy_prob={"increasing_horizon": 1.0}, initial_horizon=8, horizon_step=4, max_horizon=30)
    assert ix.current_horizon == 8
    ix.increase_horizon(3)
    assert ix.current_horizon == 20
    ix.increase_horizon(6)
    assert ix.current_horizon == 30  # 32 -> max_horizon
    ix.increase_horizon(1000)
    assert ix.current_horizon == 30
    ix.increase_horizon_to(12)
    assert ix.current_horizon == 12
    ix.increase_horizon_to(31)
    assert ix.current_horizon == 30


def test_constructor_validates_the_tables():
    from tacorl_amd.data.replay import TransitionIndex

    ok = dict(goal_strategy_prob={"geometric": 0.5, "similar_robot_obs": 0.5})
    TransitionIndex(G.ep, n_frames=60, nn_steps_from_step={3: [59, 0]}, **ok)
    with pytest.raises(ValueError):
        TransitionIndex(G.ep, n_frames=60, nn_steps_from_step={3: [60]}, **ok)   # a neighbour id outside the dataset
    with pytest.raises(ValueError):
        TransitionIndex(G.ep, n_frames=60, nn_steps_from_step={3: [-1]}, **ok)
    with pytest.raises(ValueError):
        TransitionIndex(G.ep, n_frames=60, nn_steps_from_step={60: [1]}, **ok)
    with pytest.raises(ValueError):
        TransitionIndex([[0, 17], [17, 30]], **ok)                               # overlapping episodes (a shared frame)
    with pytest.raises(ValueError):
        TransitionIndex([[18, 30], [0, 17]], **ok)                               # unsorted
    with pytest.raises(ValueError):
        TransitionIndex(G.ep, n_frames=59, **ok)                                 # an episode end outside the dataset
    with pytest.raises(ValueError):
        TransitionIndex(G.ep, goal_strategy_prob={"geometric": 0.5, "random": 0.4})
    with pytest.raises(NotImplementedError):
        TransitionIndex(G.ep, goal_strategy_prob={"task_future": 1.0})
    with pytest.raises(NotImplementedError):
        TransitionIndex(G.ep, filter_by_tasks=True, **ok)


def test_transition_augmentation_draws_three_independent_tables():
    import torch

    from tacorl_amd.data.augment import AugmentSpec, draw_transition_batch_augmentation

    specs = {"rgb_static": AugmentSpec(pad=6, resize=(128, 128)), "rgb_gripper": AugmentSpec(pad=4)}
    aug = draw_transition_batch_augmentation(specs, 32, "cpu", torch.Generator().manual_seed(0))
    assert set(aug) == {"obs", "next", "goal", "pad", "resize"}
    assert aug["pad"] == {"rgb_static": 6, "rgb_gripper": 4} and aug["resize"] == {"rgb_static": (128, 128)}
    for cam in specs:
        t = [aug[r][cam] for r in ("obs", "next", "goal")]
        assert all(x["shift"].shape == (32, 2) and x["shift"].dtype == torch.int32 and x["jitter"].shape == (32, 8) for x in t)
        assert not torch.equal(t[0]["jitter"], t[1]["jitter"]) and not torch.equal(t[1]["jitter"], t[2]["jitter"])
        assert not torch.equal(t[0]["shift"], t[1]["shift"]) and not torch.equal(t[0]["shift"], t[2]["shift"])
