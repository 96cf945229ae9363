"""D4RLWindowIndex (tacorl_amd/data/d4rl_replay.py) against the items recorded from the unmodified reference D4RLPlayDataset
(tests/golden/d4rl_window_sampler.npz, tools/gen_d4rl_window_golden.py), the episode rules on small hand-written flag tables,
the draws, the rejected options, and the binding row of the sampler kernel.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.d4rl_window_util import VARIANTS, D4rlWindowGolden, coverage, synthetic_dataset

G = D4rlWindowGolden()


def _index(**kw):
    from tacorl_amd.data.d4rl_replay import D4RLWindowIndex

    return D4RLWindowIndex(**kw)


def _flags(n, timeouts=(), terminals=()):
    t, d = np.zeros(n, bool), np.zeros(n, bool)
    t[list(timeouts)], d[list(terminals)] = True, True
    return dict(timeouts=t, terminals=d)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_index_reproduces_the_recorded_items(variant):
    v, ix = G.variants[variant], G.index(variant)
    assert G.cfg["variants"][variant] == VARIANTS[variant]
    assert len(ix) == int(v["len"]) and np.array_equal(ix.ep, v["ep"])
    s = ix.sample(None, G.draws(variant), G.dataset["observations"], G.dataset["actions"])
    assert s["observations"].dtype == s["actions"].dtype == s["goal"].dtype == np.float32 and s["goal_reached"].dtype == np.bool_
    assert np.array_equal(s["observations"], v["observations"]) and np.array_equal(s["actions"], v["actions"])
    assert np.array_equal(s["window"], v["window"]) and np.array_equal(s["start"], ix.episode_lookup[v["idx"]])
    if VARIANTS[variant]["include_goal"]:
        assert np.array_equal(s["goal"], v["goal"]) and np.array_equal(s["goal_reached"], v["goal_reached"])
    cov = coverage(variant, v, v["ep"], VARIANTS[variant])
    assert cov and all(cov.values()), cov


def test_fixture_dataset_is_the_synthetic_one():
    d = synthetic_dataset()
    assert all(np.array_equal(d[k], G.dataset[k]) and d[k].dtype == G.dataset[k].dtype for k in d)
    ends = np.flatnonzero(d["timeouts"] | d["terminals"])
    assert ends.tolist() == [39, 48, 73, 74, 134, 151] and len(d["timeouts"]) == 157
    assert (d["timeouts"] & d["terminals"]).sum() == 1 and d["timeouts"].sum() > 1 and d["terminals"].sum() > 1
    ix = G.index("lmp_8_16")
    assert ix.ep.tolist() == [[0, 39], [49, 73], [75, 134], [135, 151]] and len(ix) == 78
    assert (ix.episode_lookup == 135).sum() == 1 and ix.episode_lookup[-1] == 135  # the 17-frame episode: one item


def test_step_with_both_flags_is_one_end():
    ix = _index(**_flags(60, timeouts=[29, 59], terminals=[29]), min_window_size=4, max_window_size=8)
    assert ix.ep.tolist() == [[0, 29], [30, 59]]
    assert ix.episode_lookup.tolist() == list(range(0, 22)) + list(range(30, 52))


def test_episode_kept_only_when_longer_than_min_plus_one():
    # end - start == min (length min + 1) is dropped, == min + 1 is kept
    f = _flags(40, timeouts=[19, 24, 30])  # [0,19] kept, [20,24]: 4 == min dropped, [25,30]: 5 == min + 1 kept
    ix = _index(**f, min_window_size=4, max_window_size=5)
    assert ix.ep.tolist() == [[0, 19], [25, 30]]
    assert ix.episode_lookup.tolist() == list(range(0, 15)) + [25]  # range(start, end + 1 - max)


def test_kept_episode_shorter_than_max_has_no_item_and_trailing_frames_are_ignored():
    f = _flags(50, terminals=[19, 25])  # [20,25]: kept (5 > 4) but 6 frames < max 8; frames 26..49 follow no end
    ix = _index(**f, min_window_size=4, max_window_size=8)
    assert ix.ep.tolist() == [[0, 19], [20, 25]]
    assert ix.episode_lookup.tolist() == list(range(0, 12)) and len(ix) == 12
    assert ix.episode_lookup.max() + 8 - 1 <= 19 and ix.n_frames == 50


def test_episode_end_at_or_below_max_window_raises():
    with pytest.raises(ValueError):  # the reference asserts end_idx > max_window_size on the absolute index
        _index(**_flags(40, timeouts=[8, 39]), min_window_size=4, max_window_size=8)
    _index(**_flags(40, timeouts=[9, 39]), min_window_size=4, max_window_size=8)
    with pytest.raises(ValueError):
        _index(**_flags(40), min_window_size=4, max_window_size=8)  # no end at all: no episode


def test_huge_displacement_gives_the_episode_end():
    ix = G.index("tacorl_8_16")
    n = 16
    d = ix.draw(n, np.random.default_rng(0))
    d["disp"][:] = 2 ** 62
    d["disp"][1] = 2 ** 63 - 1
    s = ix.sample(None, d, G.dataset["observations"], G.dataset["actions"])
    assert np.array_equal(s["goal_step"], ix.episode_end(s["start"]))
    assert np.array_equal(s["goal"], G.dataset["observations"][s["goal_step"], :2])


def test_goal_step_is_the_clipped_product():
    ix = G.index("tacorl_8_16")
    d = ix.draw(500, np.random.default_rng(1))
    s = ix.sample(None, d, G.dataset["observations"], G.dataset["actions"])
    end = ix.episode_end(s["start"])
    assert np.array_equal(s["goal_step"], np.minimum(end, s["start"] + (d["window"] - 1) * d["disp"]))
    assert (s["goal_step"] == end).any() and (s["goal_step"] < end).any()
    # padding: observations repeat the window's last row, actions are zero rows
    k = int(np.argmin(d["window"]))
    w = int(d["window"][k])
    assert w < 16 and np.array_equal(s["observations"][k, w:], np.repeat(s["observations"][k, w - 1: w], 16 - w, 0))
    assert not s["actions"][k, w:].any() and s["actions"][k, :w].all()


def test_draw_ranges():
    import torch

    for variant in ("tacorl_8_16", "tacorl_8_8"):
        ix = G.index(variant)
        d = ix.draw(4000, np.random.default_rng(2))
        assert set(d) == {"idx", "window", "disp"} and all(v.dtype == np.int64 and v.shape == (4000,) for v in d.values())
        assert d["idx"].min() == 0 and d["idx"].max() == len(ix) - 1 and d["disp"].min() == 1
        assert d["window"].min() == ix.min and d["window"].max() == ix.max
        t = ix.draw_device(4000, "cpu", torch.Generator().manual_seed(3))
        assert all(v.dtype == torch.int64 and v.shape == (4000,) for v in t.values())
        assert int(t["idx"].min()) >= 0 and int(t["idx"].max()) < len(ix) and int(t["disp"].min()) >= 1
        assert int(t["window"].min()) == ix.min and int(t["window"].max()) == ix.max
        assert abs(float(t["disp"].double().mean()) - 1 / 0.3) < 0.3  # geometric(0.3)
    with pytest.raises(IndexError):
        ix.sample(None, {"idx": np.array([len(ix)]), "window": np.array([8]), "disp": np.array([1])}, G.dataset["observations"],
                  G.dataset["actions"])


def test_rejected_options_raise():
    from tacorl_amd.data.d4rl_replay import D4RLDataModule

    f = dict(timeouts=G.dataset["timeouts"], terminals=G.dataset["terminals"])
    with pytest.raises(NotImplementedError):
        _index(**f, goal_augmentation=True)
    with pytest.raises(NotImplementedError):
        _index(**f, pad=False)  # 8..16 cannot be collated unpadded
    _index(**f, pad=False, min_window_size=8, max_window_size=8)
    with pytest.raises(NotImplementedError):
        _index(**f, min_window_size=1, max_window_size=8)
    with pytest.raises(ValueError):
        _index(**f, min_window_size=9, max_window_size=8)
    with pytest.raises(ValueError):
        _index(**f, goal_sampling_prob=0.0)
    arrays = dict(G.dataset)
    with pytest.raises(NotImplementedError):
        D4RLDataModule({"arrays": arrays}, transform_manager={"transforms": {"train": {"observations": [{"_target_": "x.NormalizeVector"}]}}})
    with pytest.raises(ValueError):
        D4RLDataModule({"min_window_size": 8})  # neither path nor arrays
    with pytest.raises(TypeError):
        D4RLDataModule({"arrays": arrays, "window": 3})
    # the reference's composed config: image transforms only, d4rl_env and num_workers accepted
    dm = D4RLDataModule({"arrays": arrays, "d4rl_env": "antmaze-large-diverse-v0", "_target_": "tacorl.datamodule.dataset."
                         "d4rl_play_dataset.D4RLPlayDataset", "include_goal": True}, batch_size=64, num_workers=4,
                        transform_manager={"transforms": {"train": {"rgb_static": [{"_target_": "torchvision.transforms.Resize"}]}}})
    assert dm.replay is None  # nothing touches a device before setup()


def test_from_npz_reads_the_d4rl_key_names(tmp_path):
    from tacorl_amd.data.d4rl_replay import HbmD4RLReplay

    np.savez(tmp_path / "bad.npz", observations=G.dataset["observations"])
    with pytest.raises(KeyError):
        HbmD4RLReplay.from_npz(tmp_path / "bad.npz")


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
    name = "tacorl_sample_d4rl_windows"
    m = re.search(r"([A-Za-z_][A-Za-z_0-9 ]*?)\b" + name + r"\s*\(([^;]*)\)\s*;", txt, flags=re.S)
    assert m, name
    res, args = _lib._SIGS[name]
    assert ctype_of(m.group(1)) is res
    got = [ctype_of(a) for a in m.group(2).split(",")]
    assert got == list(args), [(i, a.strip()) for i, (a, x, y) in enumerate(zip(m.group(2).split(","), got, args)) if x is not y]
    assert len(args) == 27 and [i for i, a in enumerate(args) if a is C.c_float] == [17]  # the threshold
    assert hasattr(_lib.lib(), name)
