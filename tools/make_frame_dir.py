"""Write a synthetic dataset directory in the reference's layout (datamodule/dataset/play_dataset.py; CALVIN's): one
np.savez_compressed file per frame, `episode_<step, 7 digits>.npz` with rgb_static, rgb_gripper, rel_actions_world,
rel_actions_gripper, robot_obs and scene_obs, the episode table as ep_start_end_ids.npy and / or split.json, step numbers
with an offset and gaps between episodes.  Every array of a step is a function of (seed, step) alone, so a test rebuilds
the directory a fixture was recorded on from its seed.  Used by the tests, tools/gen_frame_dir_golden.py and
tools/time_frame_dir.py.

    python tools/make_frame_dir.py OUT --frames 4000 --hw 200 200 --episodes 8
"""
import argparse
import json
import os

import numpy as np

CAMERAS = ("rgb_static", "rgb_gripper")


def step_arrays(seed, step, hw, gripper_hw=None, smooth=False):
    """The arrays of one step.  smooth: frames with low-frequency content (they compress like camera frames, not like noise)."""
    rs = np.random.RandomState((int(seed) * 1000003 + int(step)) % (2**31 - 1))
    out = {}
    for cam, (h, w) in zip(CAMERAS, (hw, gripper_hw or hw)):
        if smooth:
            yy, xx = np.mgrid[0:h, 0:w]
            a, b, c = rs.uniform(0.02, 0.2, size=3)
            img = np.stack([127 + 120 * np.sin(a * xx + b * yy + k + c * step) for k in range(3)], -1)
            out[cam] = np.clip(img + rs.randint(-1, 2, size=img.shape), 0, 255).astype(np.uint8)
        else:
            out[cam] = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    for k in ("rel_actions_world", "rel_actions_gripper"):
        a = rs.uniform(-1, 1, size=7).astype(np.float32)
        a[-1] = 1.0 if a[-1] >= 0 else -1.0
        out[k] = a
    out["robot_obs"] = rs.uniform(-1, 1, size=15).astype(np.float32)
    out["scene_obs"] = rs.uniform(-1, 1, size=24).astype(np.float32)
    return out


def episodes_of(n_frames, n_episodes, offset=1000, gap=10):
    """n_episodes episodes of about n_frames / n_episodes steps each, the first at `offset`, `gap` unused steps between two."""
    per, ep, s = max(int(n_frames) // int(n_episodes), 1), [], int(offset)
    for _ in range(int(n_episodes)):
        ep.append([s, s + per - 1])
        s += per + int(gap)
    return ep


def make_frame_dir(root, train_episodes, val_episodes=None, hw=(8, 8), gripper_hw=None, seed=0, table="npy", prefix="episode_",
                   n_digits=7, smooth=False, split_keys=("training", "validation")):
    """Writes the frames of every episode of both tables into `root` and the tables as `table` says: "npy"
    (ep_start_end_ids.npy = train_episodes), "split" (split.json with both) or "both".  Returns {step: its arrays}."""
    os.makedirs(root, exist_ok=True)
    data = {}
    for s, e in list(train_episodes) + list(val_episodes or []):
        for step in range(int(s), int(e) + 1):
            data[step] = arr = step_arrays(seed, step, hw, gripper_hw, smooth)
            np.savez_compressed(os.path.join(root, f"{prefix}{step:0{n_digits}d}.npz"), **arr)
    if table in ("npy", "both"):
        np.save(os.path.join(root, "ep_start_end_ids.npy"), np.asarray(train_episodes, dtype=np.int64))
    if table in ("split", "both"):
        with open(os.path.join(root, "split.json"), "w") as f:
            json.dump({split_keys[0]: [list(map(int, e)) for e in train_episodes],
                       split_keys[1]: [list(map(int, e)) for e in (val_episodes or [])]}, f)
    return data


def stacked(data, episodes, key):
    """The arrays `key` of the steps the episodes cover, in step order: what the compacted table holds."""
    return np.stack([data[s][key] for a, b in episodes for s in range(int(a), int(b) + 1)])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("out")
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--episodes", type=int, default=4)
    ap.add_argument("--hw", type=int, nargs=2, default=(200, 200))
    ap.add_argument("--gripper-hw", type=int, nargs=2, default=None)
    ap.add_argument("--offset", type=int, default=1000)
    ap.add_argument("--gap", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--table", choices=("npy", "split", "both"), default="npy")
    ap.add_argument("--noise", action="store_true", help="uniform noise frames instead of smooth ones")
    a = ap.parse_args()
    ep = episodes_of(a.frames, a.episodes, a.offset, a.gap)
    val = [[ep[-1][1] + a.gap + 1, ep[-1][1] + a.gap + max(a.frames // a.episodes // 4, 40)]] if a.table != "npy" else None
    make_frame_dir(a.out, ep, val, tuple(a.hw), tuple(a.gripper_hw) if a.gripper_hw else None, a.seed, a.table, smooth=not a.noise)
    print(f"{a.out}: {sum(e - s + 1 for s, e in ep)} training frames in {len(ep)} episodes from step {ep[0][0]}")


if __name__ == "__main__":
    main()
