"""The host side of the resident play replay (tacorl_amd/data/play_replay.py), without a GPU: PlayIndex.draw_device's
distributions and shared constants, the table validation the unchecked device gathers rely on, the ABI row of the sampler
entry point, and PlayDataModule's handling of the reference's configs."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tacorl_amd.data.replay import PlayIndex


def test_device_draws_follow_the_reference_distributions():
    """The bounds of tests/test_sampler_cpu.py::test_draws_follow_the_reference_distributions, on draw_device."""
    ix = PlayIndex([[0, 999]], 8, 16, goal_sampling_prob=0.3, goal_augmentation=True)
    d = ix.draw_device(20000, "cpu", torch.Generator().manual_seed(0))
    assert set(d) == {"idx", "window_size", "strategy", "disp", "noise_step", "u_choice", "u_random_state"}
    for k in ("idx", "window_size", "strategy", "disp", "noise_step"):
        assert d[k].dtype == torch.int64 and d[k].shape == (20000,), k
    for k in ("u_choice", "u_random_state"):
        assert d[k].dtype == torch.float64 and float(d[k].min()) >= 0.0 and float(d[k].max()) < 1.0, k
    assert int(d["idx"].min()) >= 0 and int(d["idx"].max()) < len(ix) and d["idx"].unique().numel() > 900
    assert int(d["window_size"].min()) == 8 and int(d["window_size"].max()) == 16
    assert abs(float(d["strategy"].double().mean()) - 0.5) < 0.02 and abs(float(d["disp"].double().mean()) - 1 / 0.3) < 0.1
    assert int(d["disp"].min()) >= 1
    assert set(d["noise_step"].unique().tolist()) == {-1, 0, 1}
    # the strategy follows p: 0.9 geometric (config/datamodule/dataset/tacorl.yaml)
    ix9 = PlayIndex([[0, 999]], 8, 16, goal_strategy_prob={"geometric": 0.9, "similar_robot_obs": 0.1})
    d9 = ix9.draw_device(20000, "cpu", torch.Generator().manual_seed(1))
    assert abs(float(d9["strategy"].double().mean()) - 0.1) < 0.02
    # the same generator state gives the same draws
    again = ix.draw_device(20000, "cpu", torch.Generator().manual_seed(0))
    assert all(torch.equal(d[k], again[k]) for k in d)


def test_what_is_no_draw_is_made_once():
    ix = PlayIndex([[0, 999]], 16, 16)  # min == max, no goal augmentation
    a, b = ix.draw_device(32, "cpu"), ix.draw_device(32, "cpu")
    assert a["window_size"] is b["window_size"] and a["noise_step"] is b["noise_step"]
    assert bool((a["window_size"] == 16).all()) and bool((a["noise_step"] == 0).all())
    assert a["idx"] is not b["idx"] and a["disp"] is not b["disp"]
    c = ix.draw_device(8, "cpu")
    assert c["window_size"] is not a["window_size"] and c["window_size"].shape == (8,)
    assert ix.draw_device(8, "cpu")["window_size"] is c["window_size"]
    var = PlayIndex([[0, 999]], 8, 16, goal_augmentation=True)
    x, y = var.draw_device(32, "cpu"), var.draw_device(32, "cpu")
    assert x["window_size"] is not y["window_size"] and x["noise_step"] is not y["noise_step"]


def _index(**kw):
    return PlayIndex([[0, 99], [100, 199]], 8, 16, **kw)


def test_table_validation_rejects_each_bad_table():
    from tacorl_amd.data.neighbours import NeighbourTable
    from tacorl_amd.data.play_replay import HbmPlayReplay, validate_play_tables

    acts = np.zeros((200, 7), np.float32)
    validate_play_tables(_index(nn_steps_from_step={5: [7, 150], 199: []}), 200)
    validate_play_tables(_index(nn_steps_from_step=NeighbourTable.from_dict({5: [7, 150], 120: []}, 200)), 200)
    rp = HbmPlayReplay({}, acts, _index(), device="cpu", batch_size=4, slots=2)  # the class builds on CPU tensors
    assert rp.tables["n_frames"] == 200 and rp.tables["last_end"] == 199 and rp.tables["lookup"].numel() == 2 * 84

    def bad(ix, n=200, match=None):
        with pytest.raises(ValueError, match=match):
            validate_play_tables(ix, n)
        with pytest.raises(ValueError, match=match):  # ... and the replay refuses to be built on it
            HbmPlayReplay({}, acts[:n], ix, device="cpu")

    bad(_index(), n=199, match="episode bounds")                       # an episode end beyond the dataset
    ix = _index()
    ix.ep = np.array([[-1, 99], [100, 199]])
    bad(ix, match="episode bounds")
    bad(PlayIndex([[100, 199], [0, 99]], 8, 16), match="sorted")      # not sorted by start
    bad(PlayIndex([[0, 120], [100, 199]], 8, 16), match="sorted")     # overlapping
    ix = _index()
    ix.episode_lookup = np.append(ix.episode_lookup, 85)              # 85 + 16 - 1 = 100 > 99
    bad(ix, match="leaves its episode")
    ix = _index()
    ix.episode_lookup[0] = -1
    bad(ix, match="leaves its episode")
    bad(_index(nn_steps_from_step={200: [3]}), match="key outside")
    bad(_index(nn_steps_from_step={-1: [3], 5: [4]}), match="key outside")
    bad(_index(nn_steps_from_step={5: [200]}), match="neighbour outside")
    bad(_index(nn_steps_from_step={5: [3, -1]}), match="neighbour outside")
    bad(_index(nn_steps_from_step=NeighbourTable.from_dict({5: [7, 250]}, 300)), match="neighbour outside")
    bad(_index(nn_steps_from_step=NeighbourTable.from_dict({250: [7]}, 300)), match="key outside")
    with pytest.raises(ValueError, match="uint8"):
        HbmPlayReplay({"rgb_static": np.zeros((200, 8, 8, 3), np.float32)}, acts, _index(), device="cpu")
    with pytest.raises(ValueError, match="slots"):
        HbmPlayReplay({}, acts, _index(), device="cpu", slots=0)
    # the dataset is as long as its shortest table: a camera of 150 frames does not cover the second episode
    with pytest.raises(ValueError, match="episode bounds"):
        HbmPlayReplay({"rgb_static": np.zeros((150, 8, 8, 3), np.uint8)}, acts, _index(), device="cpu")


def test_header_ctypes_table_agree():
    """Argument by argument: the C types of the header's prototype are the ctypes entries of the binding's row."""
    from tacorl_amd import _lib

    def ctype_of(decl):
        decl = decl.strip()
        if "*" in decl or "tacorl_stream_t" in decl:
            return C.c_void_p
        for word, ct in (("size_t", C.c_size_t), ("float", C.c_float), ("long", C.c_long), ("int", C.c_int)):
            if re.search(r"\b" + word + r"\b", decl):
                return ct
        raise AssertionError(decl)

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "tacorl_hip.h")).read(), flags=re.S)
    name = "tacorl_sample_play_windows"
    m = re.search(r"([A-Za-z_][A-Za-z_0-9 ]*?)\b" + name + r"\s*\(([^;]*)\)\s*;", txt, flags=re.S)
    assert m, name
    res, args = _lib._SIGS[name]
    assert ctype_of(m.group(1)) is res
    got = [ctype_of(a) for a in m.group(2).split(",")]
    assert got == list(args), [(i, a.strip()) for i, (a, x, y) in enumerate(zip(m.group(2).split(","), got, args)) if x is not y]
    assert len(args) == 28 and hasattr(_lib.lib(), name)


# ------------------------------------------------------------------------------------------------------ the datamodule
MODALITIES = ["actions", "rel_actions_world", "robot_obs", "scene_obs", "depth_gripper", "depth_static", "rgb_gripper", "rgb_static"]
# config/datamodule/dataset/tacorl.yaml and play_dataset.yaml of the reference, as hydra composes them
DS_TACORL = {"_target_": "tacorl.datamodule.dataset.play_dataset.PlayDataset", "_recursive_": False, "modalities": MODALITIES,
             "min_window_size": 8, "max_window_size": 16, "pad": True, "include_goal": True,
             "nn_steps_from_step_path": "~/tacorl/calvin/nn_steps_from_step.json", "goal_sampling_prob": 0.3,
             "goal_strategy_prob": {"geometric": 0.9, "similar_robot_obs": 0.1}}
DS_PLAY = {"_target_": "tacorl.datamodule.dataset.play_dataset.PlayDataset", "_recursive_": False, "modalities": MODALITIES,
           "min_window_size": 8, "max_window_size": 16, "pad": True}
# config/datamodule/{tacorl,play_lmp}.yaml
DM = {"_target_": "tacorl.datamodule.basic_data_module.BasicDataModule", "_recursive_": False, "data_dir": "~/tacorl/calvin",
      "batch_size": 64, "num_workers": 4, "val_percentage": 0.2, "train_percentage": 1.0, "shuffle_val": False}
RL_TRAIN = [{"_target_": "torchvision.transforms.Resize", "size": [8, 8]}, {"_target_": "tacorl.utils.transforms.RandomShiftsAug", "pad": 3},
            {"_target_": "tacorl.utils.transforms.ScaleImageTensor"},
            {"_target_": "tacorl.utils.transforms.ColorTransform", "contrast": 0.1, "brightness": 0.2, "hue": 0.02},
            {"_target_": "torchvision.transforms.Normalize", "mean": [0.5], "std": [0.5]}]
TM = {"transforms": {"train": {"rgb_static": RL_TRAIN, "depth_static": [{"_target_": "tacorl.utils.transforms.ColorizeDepth"}]},
                     "validation": {"rgb_static": [RL_TRAIN[0], RL_TRAIN[2], RL_TRAIN[4]]}}}


def _arrays(n=400, hw=8):
    return {"frames": {"rgb_static": np.zeros((n, hw, hw, 3), np.uint8)}, "actions": np.zeros((n, 7), np.float32),
            "ep_start_end_ids_train": [[0, 149], [150, 299]], "ep_start_end_ids_val": [[300, 399]]}


def test_datamodule_parses_the_reference_configs_and_splits():
    from tacorl_amd.data.play_replay import PlayDataModule, PlayWindowLoader

    nn = {20: [30, 40], 200: [1]}
    dm = PlayDataModule(dict(DS_TACORL, arrays=_arrays()), transform_manager=TM, nn_steps_from_step=nn, device="cpu", **DM)
    sp = dm.aug_specs["rgb_static"]  # (a camera the dataset does not hold - depth_static - is not looked at)
    assert (sp.pad, sp.brightness, sp.contrast, sp.hue, sp.prob, sp.resize) == (3, 0.2, 0.1, 0.02, 1.0, (8, 8))
    assert dm.include_goal and dm.batch_size == 64 and dm.fused is True
    dm.setup()
    ix, vix = dm.train_replay.index, dm.val_replay.index
    assert (ix.min_ws, ix.max_ws, ix.p_geom_goal, ix.train, vix.train) == (8, 16, 0.3, True, False)
    assert np.allclose(ix.p_strategy, [0.9, 0.1]) and not ix.goal_augmentation
    # items: range(s, e + 1 - max_ws) per episode; the Subset keeps the first int(len * p)
    assert len(ix) == 2 * 134 and len(vix) == int(84 * 0.2) and np.array_equal(vix.episode_lookup, np.arange(300, 316))
    assert set(ix.nn) == {20, 200} and ix.nn[20].tolist() == [30, 40]
    assert len(vix._nn_val) == 0  # no validation table given: similar_robot_obs goals fall back to a random state
    assert dm.steps_per_epoch == 268 // 64 and dm.val_steps == 1
    tl, vl = dm.train_dataloader(), dm.val_dataloader()
    assert isinstance(tl, PlayWindowLoader) and len(tl) == 4 and tl.train and tl.fused and vl.train is False and len(vl) == 1
    assert tl.aug_specs["rgb_static"].resize is None and vl.aug_specs is None  # Resize to the stored size: no stage
    assert dm.train_replay.include_goal and dm.train_replay.frames["rgb_static"] is dm.val_replay.frames["rgb_static"]
    # PlayLMP's dataset: no goal, defaults elsewhere; half of each split
    dp = PlayDataModule(dict(DS_PLAY, arrays=_arrays()), **dict(DM, train_percentage=0.5, val_percentage=0.5), device="cpu")
    dp.setup()
    assert not dp.include_goal and not dp.train_replay.include_goal
    assert len(dp.train_replay.index) == 134 and len(dp.val_replay.index) == 42
    assert np.array_equal(dp.train_replay.index.episode_lookup, np.arange(0, 134))
    assert dp.train_dataloader().aug_specs is None
    d0 = PlayDataModule(dict(DS_PLAY, arrays=_arrays()), batch_size=4, val_percentage=0.0, device="cpu")
    assert d0.val_dataloader() is None and len(d0.train_dataloader()) == 268 // 4
    # the real-world variant's overrides (config/datamodule/play_lmp_real_world.yaml)
    rw = PlayDataModule(dict(DS_PLAY, real_world=True, modalities=["rgb_static", "rel_actions_world"], min_window_size=20,
                             max_window_size=32, arrays=_arrays()), batch_size=8, device="cpu")
    rw.setup()
    assert (rw.index.min_ws, rw.index.max_ws) == (20, 32) and len(rw.index) == 2 * 118


def test_datamodule_reads_the_npz_and_the_neighbour_json(tmp_path):
    from tacorl_amd.data.neighbours import NeighbourTable
    from tacorl_amd.data.play_replay import PlayDataModule

    a = _arrays()
    np.savez(tmp_path / "play.npz", **{"frames/rgb_static": a["frames"]["rgb_static"], "actions": a["actions"],
                                       "ep_start_end_ids_train": a["ep_start_end_ids_train"],
                                       "ep_start_end_ids_val": a["ep_start_end_ids_val"]})
    NeighbourTable.from_dict({20: [30, 40]}, 400).save_json(tmp_path / "nn.json", "train")
    NeighbourTable.from_dict({310: [350]}, 400).save_json(tmp_path / "nn.json", "validation")
    ds = dict(DS_TACORL, path=str(tmp_path / "play.npz"), nn_steps_from_step_path=str(tmp_path / "nn.json"))
    dm = PlayDataModule(ds, batch_size=8, device="cpu")
    assert dm.cams == ["rgb_static"]
    dm.setup()
    assert dm.train_replay.index.nn_table.to_dict() == {20: [30, 40]} and dm.val_replay.index.nn_table.to_dict() == {310: [350]}
    assert dm.train_replay.tables["n_nn"] == 21
    tab = NeighbourTable.from_dict({7: [9]}, 400)
    dm2 = PlayDataModule(dict(ds, nn_steps_from_step=tab), batch_size=8, val_percentage=0.0, device="cpu")
    dm2.setup()
    assert dm2.index.nn_table.to_dict() == {7: [9]}  # a table given outright goes before the config's path
    np.savez(tmp_path / "bad.npz", actions=a["actions"])
    with pytest.raises(KeyError):
        PlayDataModule(dict(DS_PLAY, path=str(tmp_path / "bad.npz")), device="cpu").setup()


def test_datamodule_refuses_what_it_does_not_know():
    from tacorl_amd.data.play_replay import PlayDataModule

    ds = dict(DS_TACORL, arrays=_arrays())
    with pytest.raises(TypeError, match="window"):
        PlayDataModule(dict(ds, window=3))                      # an unknown dataset key
    with pytest.raises(TypeError, match="sampler"):
        PlayDataModule(ds, sampler="x")                         # an unknown datamodule key
    bad = {"transforms": {"train": {"rgb_static": RL_TRAIN + [{"_target_": "tacorl.utils.transforms.AddGaussianNoise", "std": 0.01}]}}}
    with pytest.raises(NotImplementedError, match="AddGaussianNoise"):
        PlayDataModule(ds, transform_manager=bad)               # a transform augment_specs does not build
    with pytest.raises(ValueError, match="path"):
        PlayDataModule(dict(ds, path="play.npz"))               # path and arrays together
    with pytest.raises(ValueError, match="path"):
        PlayDataModule(dict(DS_TACORL))                         # ... and neither
    with pytest.raises(NotImplementedError, match="pad"):
        PlayDataModule(dict(ds, pad=False))
    with pytest.raises(ValueError, match="train_percentage"):
        PlayDataModule(ds, train_percentage=1.5)
    with pytest.raises(ValueError, match="no item"):
        PlayDataModule(ds, train_percentage=0.0, device="cpu").setup()
    with pytest.raises(KeyError, match="ep_start_end_ids_val"):
        a = {k: v for k, v in _arrays().items() if k != "ep_start_end_ids_val"}
        PlayDataModule(dict(DS_PLAY, arrays=a), device="cpu").setup()
    # validation frames are not resized: a Resize away from the stored size is refused where a validation loader is asked for
    tm = {"transforms": {"train": {"rgb_static": [{"_target_": "torchvision.transforms.Resize", "size": 16}]}}}
    with pytest.raises(NotImplementedError, match="resize"):
        PlayDataModule(ds, transform_manager=tm, device="cpu").setup()
