"""Generate tests/golden/relay_sampler.npz: what the UNMODIFIED reference RILDataset.__getitem__
(datamodule/dataset/relay_imitation_learning_dataset.py:73-113) returns on tiny synthetic datasets written to a temp dir,
with every numpy draw it consumes recorded (needs the reference checkout that oracle/ref_harness.py points at).

    python tools/gen_relay_golden.py

Frame ids are encoded in the pixel values, so the fixture holds, per variant (episodes, max_low_level_window,
max_high_level_window) and for EVERY item of it: the item index, the recorded uniforms of the low-level and the high-level
np.random.choice (0.0 where the reference drew none), how many it drew, the frame ids of obs / low_level_goal /
high_level_goal / high_level_action and the action row - plus the settings.  No image, no reference source text.
The transform manager is stood in for by a function that returns the frame as loaded and counts its calls (the reference
calls it once per frame: four per item)."""
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as H  # noqa: E402

H.install_shims()
from tacorl.datamodule.dataset.relay_imitation_learning_dataset import RILDataset  # noqa: E402

# name -> (episodes, max_low_level_window, max_high_level_window)
VARIANTS = {
    "yaml_30_260": ([[0, 69], [70, 159]], 30, 260),       # config/datamodule/dataset/relay_imitation_learning.yaml
    "short_4_12": ([[0, 69], [70, 159]], 4, 12),          # both ranges non-empty away from the episode ends
    "low1_high3": ([[0, 39], [40, 52], [53, 99]], 1, 3),  # Lw = 1: the low range is always empty
    "equal_6_6": ([[0, 39], [40, 99]], 6, 6),             # Hw == Lw: the high range is always empty
    "high_below_low_8_5": ([[0, 39], [40, 99]], 8, 5),    # Hw < Lw: hmax lies before the subgoal
    "high_beyond_2_1000": ([[0, 39], [40, 99]], 2, 1000),  # Hw beyond every episode
}
ROLES = ("obs", "low_level_goal", "high_level_goal", "high_level_action")
N_MAX = 160
SEED = 1


def main():
    acts = np.random.RandomState(0).uniform(-1, 1, size=(N_MAX, 7)).astype(np.float32)
    rec, calls = [], [0]
    gen = np.random.RandomState(SEED)
    o_choice = np.random.choice

    def choice(options, *a, **kw):
        assert not a and not kw
        u = gen.uniform()
        rec.append(u)
        return options[min(int(u * len(options)), len(options) - 1)]

    def identity(data, transf_type=None):
        calls[0] += 1
        return dict(data)

    fid = lambda o: int(o["rgb_static"][0, 0, 0]) + 256 * int(o["rgb_static"][0, 0, 1])  # noqa: E731
    out = {}
    np.random.choice = choice
    try:
        for name, (ep, lw, hw) in VARIANTS.items():
            n = max(e for _, e in ep) + 1
            with tempfile.TemporaryDirectory() as d:
                d = Path(d)
                for i in range(n):
                    img = np.zeros((2, 2, 3), np.uint8)
                    img[..., 0], img[..., 1] = i % 256, i // 256
                    np.savez(d / f"episode_{i:07d}.npz", rgb_static=img, rel_actions_world=acts[i])
                np.save(d / "ep_start_end_ids.npy", np.array(ep))
                ds = RILDataset(data_dir=d, modalities=["rgb_static", "rel_actions_world"], max_low_level_window=lw,
                                max_high_level_window=hw, transform_manager=identity)
                cols = {k: [] for k in ("idx", "u_low", "u_high", "n_draws", "actions") + ROLES}
                for idx in range(len(ds)):
                    rec.clear()
                    calls[0] = 0
                    it = ds[idx]
                    assert calls[0] == 4 and len(rec) <= 2 and set(it) == set(ROLES) | {"low_level_action"}, (calls, rec, list(it))
                    ids = {r: fid(it[r]) for r in ROLES}
                    # which call a single recorded uniform belongs to: the low-level one comes first and is made exactly
                    # when [step + 1, subgoal) is not empty
                    low_drawn = ids["high_level_action"] - ids["obs"] - 1 > 0
                    u = list(rec)
                    u_low = u.pop(0) if low_drawn else 0.0
                    u_high = u.pop(0) if u else 0.0
                    assert not u
                    for k, val in (("idx", idx), ("u_low", u_low), ("u_high", u_high), ("n_draws", len(rec)),
                                   ("actions", np.asarray(it["low_level_action"]))):
                        cols[k].append(val)
                    for r in ROLES:
                        cols[r].append(ids[r])
                v = {k: np.asarray(c) for k, c in cols.items()}
                v["len"] = np.array(len(ds))
                print(name, "len", len(ds), "draws per item:", np.bincount(v["n_draws"], minlength=3).tolist())
                out.update({f"{name}/{k}": a for k, a in v.items()})
    finally:
        np.random.choice = o_choice
    out["all_actions"] = acts
    out["cfg"] = np.array(json.dumps({"roles": ROLES, "variants": {k: list(v) for k, v in VARIANTS.items()}}))
    path = os.path.join(ROOT, "tests", "golden", "relay_sampler.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) / 1e3, "kB")


if __name__ == "__main__":
    main()
