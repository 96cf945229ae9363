"""RelayIndex (tacorl_amd/data/relay_replay.py) against the items the reference's RILDataset returned for recorded draws
(tests/golden/relay_sampler.npz), the ranges of its own draws, the constructor's table validation, the four-role
augmentation draw and RILDataModule's config checks.  No GPU."""
import numpy as np
import pytest
import torch

from tests.relay_util import EXPECTED, ROLES, RelayGolden, extreme_draws

G = RelayGolden()
VARIANTS = list(G.variants)


def test_fixture_has_all_six_variants():
    got = [(ep.tolist(), lw, hw) for ep, lw, hw in G.settings.values()]
    assert got == EXPECTED
    from tacorl_amd.modules.relay_imitation_learning.engine import SLOTS

    assert tuple(G.cfg["roles"]) == ROLES == tuple(SLOTS)
    for name, v in G.variants.items():
        assert np.array_equal(v["idx"], np.arange(int(v["len"]))), name  # every item of the variant


@pytest.mark.parametrize("variant", VARIANTS)
def test_sample_equals_the_reference_dataset(variant):
    v = G.variants[variant]
    ep, lw, hw = G.settings[variant]
    ix = G.index(variant)
    assert len(ix) == int(v["len"]) == sum(max(e + 1 - lw - s, 0) for s, e in ep)
    d = G.draws(variant)
    s = ix.sample(d["idx"], d)
    for r in ROLES:
        assert np.array_equal(s[r], v[r]), (r, s[r], v[r])
    assert np.array_equal(G.actions[s["step"]], v["actions"])
    assert np.array_equal(ix.sample(None, d)["high_level_goal"], v["high_level_goal"])  # idx taken from the draws
    # the reference drew exactly where a range was not empty
    step, sub = s["obs"], s["high_level_action"]
    end = ix.episode_end(step)
    hmax = np.minimum(end, step + hw)
    assert np.array_equal(v["n_draws"], (sub - step - 1 > 0).astype(int) + (hmax - sub > 0).astype(int))
    # the last item of every episode is there: its subgoal is the episode end
    for s0, e in ep:
        if e + 1 - lw > s0:
            assert (step == e - lw).any() and (sub[step == e - lw] == e).all()


def test_fixture_covers_every_branch():
    n = {k: np.bincount(v["n_draws"], minlength=3) for k, v in G.variants.items()}
    assert n["low1_high3"][2] == 0 and n["low1_high3"][0] > 0 and n["low1_high3"][1] > 0  # Lw = 1: the low range is empty
    assert n["equal_6_6"].tolist()[0::2] == [0, 0] and n["high_below_low_8_5"].tolist()[0::2] == [0, 0]  # high range empty
    v = G.variants["high_below_low_8_5"]
    assert (v["high_level_goal"] < v["high_level_action"]).any()  # hmax before the subgoal
    assert n["yaml_30_260"][2] > 0 and n["high_beyond_2_1000"][2] > 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_fresh_draws_stay_inside_the_dataset_and_the_episode(variant):
    ix = G.index(variant)
    d = extreme_draws(ix, 5000, 3)
    d["idx"][:4] = [0, 0, len(ix) - 1, len(ix) - 1]
    s = ix.sample(None, d)
    step, low, high, sub = (s[r] for r in ROLES)
    end = ix.episode_end(step)
    start = ix.ep[np.searchsorted(ix.ep[:, 0], step, side="right") - 1, 0]
    for a in (step, low, high, sub):
        assert a.min() >= 0 and a.max() < ix.n_frames and (a >= start).all() and (a <= end).all()
    assert (step < low).all() and (low <= sub).all() and (high <= end).all()
    assert np.array_equal(sub, np.minimum(end, step + ix.low_window))
    if ix.low_window > 1:
        assert (low < sub).all()  # the upper bound of the choice is exclusive
        assert low[0] == step[0] + 1 and low[1] == sub[1] - 1  # u = 0 and u -> 1


def test_draws_stay_inside_their_ranges():
    ix = G.index("short_4_12")
    n = 100_000
    d = ix.draw(n, np.random.default_rng(0))
    t = ix.draw_device(n, "cpu", torch.Generator().manual_seed(0))
    assert t["idx"].dtype == torch.int64 and t["u_low"].dtype == t["u_high"].dtype == torch.float64
    for x in (d, {k: v.numpy() for k, v in t.items()}):
        assert set(x) == {"idx", "u_low", "u_high"} and x["idx"].dtype == np.int64 and x["u_low"].dtype == np.float64
        assert x["idx"].min() == 0 and x["idx"].max() == len(ix) - 1
        for k in ("u_low", "u_high"):
            # uniform on [0, 1): the mean's standard error at n = 1e5 is 9.1e-4; bound at 5 sigma
            assert x[k].min() >= 0.0 and x[k].max() < 1.0 and abs(x[k].mean() - 0.5) < 4.6e-3
        assert not np.array_equal(x["u_low"], x["u_high"])


def test_percentage_shortens_the_index():
    full = G.index("yaml_30_260")
    for p in (1.0, 0.5, 0.1, 0.015):
        ix = G.index("yaml_30_260", percentage=p)
        assert len(ix) == int(len(full) * p) and np.array_equal(ix.episode_lookup, full.episode_lookup[: len(ix)])
    with pytest.raises(ValueError):
        G.index("yaml_30_260", percentage=0.001)  # no item left


def test_constructor_validates_the_tables():
    from tacorl_amd.data.relay_replay import RelayIndex

    RelayIndex([[0, 39], [40, 99]], n_frames=100, max_low_level_window=6, max_high_level_window=6)
    with pytest.raises(ValueError):
        RelayIndex([[40, 99], [0, 39]], max_low_level_window=6)                 # unsorted
    with pytest.raises(ValueError):
        RelayIndex([[0, 40], [40, 99]], max_low_level_window=6)                 # overlapping (a shared frame)
    with pytest.raises(ValueError):
        RelayIndex([[0, 39], [40, 99]], n_frames=99, max_low_level_window=6)    # an episode end outside the dataset
    with pytest.raises(ValueError):
        RelayIndex([[-1, 39], [40, 99]], max_low_level_window=6)
    with pytest.raises(ValueError):
        RelayIndex([[0, 39], [40, 99]], max_low_level_window=0)
    with pytest.raises(ValueError):
        RelayIndex([[0, 39], [40, 99]], max_low_level_window=6, max_high_level_window=0)
    with pytest.raises(ValueError):
        RelayIndex([[0, 5], [6, 99]], max_low_level_window=6)                   # the reference's assert: end 5 <= Lw 6
    with pytest.raises(ValueError):
        RelayIndex([[10, 20], [30, 45]], max_low_level_window=20)               # every episode shorter than Lw + 1: no item
    with pytest.raises(ValueError):
        RelayIndex(np.zeros((0, 2)), max_low_level_window=6)


def test_ril_augmentation_draws_four_independent_tables():
    from tacorl_amd.data.augment import AugmentSpec, draw_ril_batch_augmentation

    specs = {"rgb_static": AugmentSpec(pad=6, resize=(128, 128)), "rgb_gripper": AugmentSpec(pad=4)}
    aug = draw_ril_batch_augmentation(specs, 32, "cpu", torch.Generator().manual_seed(0))
    assert set(aug) == set(ROLES) | {"pad", "resize"}
    assert aug["pad"] == {"rgb_static": 6, "rgb_gripper": 4} and aug["resize"] == {"rgb_static": (128, 128)}
    for cam in specs:
        t = [aug[r][cam] for r in ROLES]
        assert all(x["shift"].shape == (32, 2) and x["shift"].dtype == torch.int32 and x["jitter"].shape == (32, 8) for x in t)
        for i in range(4):
            for j in range(i + 1, 4):
                assert not torch.equal(t[i]["jitter"], t[j]["jitter"]) and not torch.equal(t[i]["shift"], t[j]["shift"])


def _arrays(n=100, hw=8):
    return {"frames": {"rgb_static": np.zeros((n, hw, hw, 3), np.uint8)}, "actions": np.zeros((n, 7), np.float32),
            "ep_start_end_ids_train": [[0, 59]], "ep_start_end_ids_val": [[60, 99]]}


RL_TRAIN = [{"_target_": "torchvision.transforms.Resize", "size": [8, 8]}, {"_target_": "tacorl.utils.transforms.RandomShiftsAug", "pad": 3},
            {"_target_": "tacorl.utils.transforms.ScaleImageTensor"},
            {"_target_": "tacorl.utils.transforms.ColorTransform", "contrast": 0.1, "brightness": 0.2, "hue": 0.02},
            {"_target_": "torchvision.transforms.Normalize", "mean": [0.5], "std": [0.5]}]


def test_datamodule_checks_its_config():
    from tacorl_amd.data import RILDataModule
    from tacorl_amd.data.relay_replay import augment_specs

    ds = {"_target_": "tacorl.datamodule.dataset.relay_imitation_learning_dataset.RILDataset", "_recursive_": False,
          "modalities": ["rgb_static", "rel_actions_world"], "action_type": "rel_actions_world", "n_digits": None, "transf_type": "train",
          "max_low_level_window": 5, "max_high_level_window": 20, "arrays": _arrays()}
    tm = {"transforms": {"train": {"rgb_static": RL_TRAIN, "depth_static": [{"_target_": "tacorl.utils.transforms.ColorizeDepth"}]},
                         "validation": {"rgb_static": [RL_TRAIN[0], RL_TRAIN[2], RL_TRAIN[4]]}}}
    dm = RILDataModule(ds, batch_size=4, train_percentage=0.5, val_percentage=0.5, transform_manager=tm, num_workers=4,
                       pin_memory=True, shuffle_val=False, _target_="tacorl.datamodule.basic_data_module.BasicDataModule")
    sp = dm.aug_specs["rgb_static"]  # (a camera the dataset does not hold - depth_static - is not looked at)
    assert (sp.pad, sp.brightness, sp.contrast, sp.hue, sp.prob, sp.resize) == (3, 0.2, 0.1, 0.02, 1.0, (8, 8))
    assert augment_specs(None, ["rgb_static"]) == {"rgb_static": None}
    with pytest.raises(TypeError):
        RILDataModule(dict(ds, window=3))
    with pytest.raises(TypeError):
        RILDataModule(ds, sampler="x")
    with pytest.raises(ValueError):
        RILDataModule({k: v for k, v in ds.items() if k != "arrays"})  # neither path nor arrays
    bad = {"transforms": {"train": {"rgb_static": RL_TRAIN + [{"_target_": "tacorl.utils.transforms.AddGaussianNoise", "std": 0.01}]}}}
    with pytest.raises(NotImplementedError, match="AddGaussianNoise"):
        RILDataModule(ds, transform_manager=bad)
    bad = {"transforms": {"train": {"rgb_static": [{"_target_": "torchvision.transforms.Normalize", "mean": [0.4], "std": [0.2]}]}}}
    with pytest.raises(NotImplementedError, match="Normalize"):
        RILDataModule(ds, transform_manager=bad)
    # the tables are built on setup (here on the CPU device: no kernel runs before a batch is asked for)
    dm.device = "cpu"
    dm.setup()
    assert len(dm.train_replay.index) == int(55 * 0.5) and len(dm.val_replay.index) == int(35 * 0.5)
    assert dm.steps_per_epoch == 27 // 4 and dm._train_specs["rgb_static"].resize is None  # Resize to the stored size: no stage
    assert len(dm.train_dataloader()) == 6 and dm.val_dataloader().train is False
    dm0 = RILDataModule(ds, batch_size=4, val_percentage=0.0, device="cpu")
    assert dm0.val_dataloader() is None and dm0.train_dataloader().aug_specs is None
