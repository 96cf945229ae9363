"""Generate tests/golden/frame_dir.npz: what the UNMODIFIED reference PlayDataset.__getitem__ (datamodule/dataset/
play_dataset.py:115-169) returns on a small dataset directory in its own layout, with every numpy draw it consumes recorded
(needs the reference checkout that oracle/ref_harness.py points at).

    python tools/gen_frame_dir_golden.py

The directory (tools/make_frame_dir.py, rebuilt by the tests in tmp_path from the seed kept in the fixture): 2 training
episodes of 30 frames of 8 x 8, two cameras, step numbers from 1000 with a gap of 10 between the episodes, a validation
episode behind them, nn_steps_from_step.json keyed by step number.  The dataset is constructed twice - on
ep_start_end_ids.npy alone, then with split.json beside it - and must return the same items.  The fixture holds, per item:
the item index, the named draws, the window's step numbers (padded), the uint8 frames of both cameras before transforms,
the actions after padding, the goal's step number and frames, disp and window_size - plus the settings.  Data only."""
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as H  # noqa: E402
from tools.make_frame_dir import make_frame_dir  # noqa: E402

H.install_shims()
from tacorl.datamodule.dataset.play_dataset import PlayDataset  # noqa: E402

TRAIN_EP, VAL_EP = [[1000, 1029], [1040, 1069]], [[1080, 1099]]
HW, SEED, MIN_WS, MAX_WS, P_GEOM, ITEMS = (8, 8), 7, 4, 8, 0.3, 24
STRATEGY = {"geometric": 0.6, "similar_robot_obs": 0.4}
CAMS = ["rgb_static", "rgb_gripper"]
_steps = [s for a, b in TRAIN_EP for s in range(a, b)]  # the keys of the reference's table: no episode end step
NN = {str(s): [int(_steps[i]) for i in np.random.RandomState(s).randint(0, len(_steps), size=s % 4)] for s in _steps}


class IdentityTransforms:  # the transform manager is out of this fixture's scope: frames pass through as float tensors
    def __call__(self, inp, transf_type="train", device="cpu"):
        return {k: torch.as_tensor(np.asarray(v)).float() for k, v in inp.items()}


def record(d, draws_of):
    """The items of PlayDataset on directory d for the item indices and generator state of draws_of()."""
    rec, files = [], []
    gen, idxs = draws_of()
    o_randint, o_choice, o_rng = np.random.randint, np.random.choice, np.random.default_rng

    def randint(low, high=None, *a, **kw):
        v = gen.randint(low, high)
        rec.append(("randint", float(v)))
        return v

    def choice(options, p=None, *a, **kw):
        u = gen.uniform()
        rec.append(("choice_u", u))
        options = list(options)
        if p is None:
            return options[min(int(u * len(options)), len(options) - 1)]
        return options[int(np.searchsorted(np.cumsum(p), u, side="right").clip(0, len(options) - 1))]

    class FakeRng:
        def geometric(self, p):
            v = gen.geometric(p)
            rec.append(("geometric", float(v)))
            return v

    np.random.randint, np.random.choice, np.random.default_rng = randint, choice, lambda *a, **k: FakeRng()
    try:
        ds = PlayDataset(data_dir=Path(d), modalities=CAMS + ["rel_actions_world"], train=True, real_world=True,
                         min_window_size=MIN_WS, max_window_size=MAX_WS, pad=True, transform_manager=IdentityTransforms(),
                         include_goal=True, goal_augmentation=False, goal_sampling_prob=P_GEOM, goal_strategy_prob=dict(STRATEGY),
                         nn_steps_from_step_path=str(Path(d) / "nn_steps_from_step.json"))
        get_file = ds.get_file
        ds.get_file = lambda file_idx, transform=True: (files.append(int(file_idx)), get_file(file_idx, transform))[1]
        cols = {k: [] for k in ("idx", "window_size", "strategy", "disp_draw", "u_choice", "steps", "goal_step", "disp", "actions")
                + tuple(f"frames/{c}" for c in CAMS) + tuple(f"goal/{c}" for c in CAMS)}
        for idx in idxs:
            rec.clear(), files.clear()
            it = ds[int(idx)]
            dr = iter(rec)
            ws = int(next(dr)[1])
            strategy = 0 if next(dr)[1] < STRATEGY["geometric"] else 1
            nxt = next(dr)
            assert next(dr, None) is None and len(files) == 1 and ws == int(it["window_size"]), (rec, files)
            start = ds.episode_lookup[int(idx)]
            steps = np.minimum(start + np.arange(MAX_WS), start + ws - 1)  # pad_with_repetition repeats the last frame
            for c in CAMS:
                fr, go = it["states"][c].numpy(), it["goal"][c].numpy()
                assert fr.shape == (MAX_WS,) + HW + (3,) and np.array_equal(fr, fr.astype(np.uint8))
                cols[f"frames/{c}"].append(fr.astype(np.uint8))
                cols[f"goal/{c}"].append(go.astype(np.uint8))
            for k, v in (("idx", int(idx)), ("window_size", ws), ("strategy", strategy), ("disp_draw", int(nxt[1]) if strategy == 0 else 1),
                         ("u_choice", float(nxt[1]) if strategy == 1 else 0.0), ("steps", steps), ("goal_step", files[0]),
                         ("disp", int(it["disp"])), ("actions", it["actions"].numpy())):
                cols[k].append(v)
        out = {k: np.asarray(v) for k, v in cols.items()}
        out["len"] = np.array(len(ds))
        return out
    finally:
        np.random.randint, np.random.choice, np.random.default_rng = o_randint, o_choice, o_rng


def main():
    def draws_of():
        gen = np.random.RandomState(123)
        return gen, gen.randint(0, 2 * (30 - MAX_WS), size=ITEMS)

    with tempfile.TemporaryDirectory() as d:
        make_frame_dir(d, TRAIN_EP, VAL_EP, HW, seed=SEED, table="npy")
        with open(os.path.join(d, "nn_steps_from_step.json"), "w") as f:
            json.dump({"train": NN}, f)
        out = record(d, draws_of)
        with open(os.path.join(d, "split.json"), "w") as f:  # the second table form, which the reference then prefers
            json.dump({"training": TRAIN_EP, "validation": VAL_EP}, f)
        again = record(d, draws_of)
        assert out.keys() == again.keys() and all(np.array_equal(out[k], again[k]) for k in out), "the table forms differ"
    assert int(out["len"]) == 2 * (30 - MAX_WS) and set(out["strategy"]) == {0, 1} and (out["window_size"] < MAX_WS).any()
    assert (out["goal_step"] >= 1040).any() and (out["steps"] < 1030).any()  # both episodes, across the gap
    out["nn"] = np.array(json.dumps(NN))
    out["cfg"] = np.array(json.dumps(dict(train_ep=TRAIN_EP, val_ep=VAL_EP, hw=HW, seed=SEED, min_ws=MIN_WS, max_ws=MAX_WS, p=P_GEOM,
                                          strategy=STRATEGY, cameras=CAMS, action_type="rel_actions_world")))
    path = os.path.join(ROOT, "tests", "golden", "frame_dir.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) / 1e3, "kB")


if __name__ == "__main__":
    main()
