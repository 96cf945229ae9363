"""Generate tests/golden/transition_sampler.npz: what the UNMODIFIED reference GoalCondReplayBufferDataset.__getitem__
(datamodule/dataset/goal_cond_replay_buffer_dataset.py:145-299) returns on a tiny synthetic dataset written to a temp
dir, with every numpy draw it consumes recorded (needs the reference checkout that oracle/ref_harness.py points at).

    python tools/gen_transition_golden.py

Frame ids are encoded in the pixel values, so the fixture holds, per goal-strategy variant and item: the item index, the
recorded draws (the strategy uniform, the geometric displacement, the uniform of the one np.random.choice over a list),
the frame ids of observation / next observation / goal, reward, terminal and the action - plus the settings (episodes,
neighbour lists, probabilities, horizons).  No image, no reference source text.
The harness lacks two names that the dataset's imports touch (utils/path.py): they are stood in for here."""
import json
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as H  # noqa: E402
from tests.transition_util import coverage  # noqa: E402  (what a variant's items must include: the test asserts the same)

H.install_shims()
_core = types.ModuleType("hydra.core")
_hc = types.ModuleType("hydra.core.hydra_config")
_hc.HydraConfig = type("HydraConfig", (), {})
_core.hydra_config = _hc
sys.modules["hydra.core"], sys.modules["hydra.core.hydra_config"] = _core, _hc
sys.modules["hydra"].core = _core
sys.modules["hydra.utils"].get_original_cwd = os.getcwd
from tacorl.datamodule.dataset.goal_cond_replay_buffer_dataset import GoalCondReplayBufferDataset  # noqa: E402

EP = [[0, 17], [18, 30], [31, 59]]  # three episodes of unequal length
N = 60
P_GEOM = 0.3
HORIZON = dict(initial_horizon=8, horizon_step=4, max_horizon=256)
NN = {str(s): [int(x) for x in np.random.RandomState(s).randint(0, N, size=s % 4)] for s in range(N)}  # 0-3 neighbours
ITEMS = 64
SEED = 1  # (with 64 items per variant, every coverage condition below holds)
# variant -> (goal_strategy_prob, epoch given to increase_horizon or None)
VARIANTS = {
    "geo_sim": ({"geometric": 0.6, "similar_robot_obs": 0.4}, None),
    "horizon": ({"increasing_horizon": 1.0}, None),
    "horizon_epoch3": ({"increasing_horizon": 1.0}, 3),
    "episode_future": ({"episode_future": 1.0}, None),
    "next_state": ({"next_state": 1.0}, None),
    "random": ({"random": 1.0}, None),
}


def main():
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        acts = np.random.RandomState(0).uniform(-1, 1, size=(N, 7)).astype(np.float32)
        for i in range(N):
            img = np.zeros((2, 2, 3), np.uint8)
            img[..., 0], img[..., 1] = i % 256, i // 256
            np.savez(d / f"episode_{i:07d}.npz", rgb_static=img, rel_actions_world=acts[i])
        np.save(d / "ep_start_end_ids.npy", np.array(EP))
        with open(d / "nn.json", "w") as f:
            json.dump({"train": NN}, f)
        rec = []
        gen = np.random.RandomState(SEED)
        o_choice, o_rng = np.random.choice, np.random.default_rng

        def choice(options, p=None, *a, **kw):
            u = gen.uniform()
            options = list(options)
            if p is None:
                rec.append(("u_choice", u))
                return options[min(int(u * len(options)), len(options) - 1)]
            rec.append(("u_strategy", u))
            return options[int(np.searchsorted(np.cumsum(p), u, side="right").clip(0, len(options) - 1))]

        class FakeRng:
            def geometric(self, p):
                v = gen.geometric(p)
                rec.append(("disp", float(v)))
                return v

        np.random.choice, np.random.default_rng = choice, lambda *a, **k: FakeRng()
        out = {}
        try:
            for variant, (probs, epoch) in VARIANTS.items():
                ds = GoalCondReplayBufferDataset(data_dir=d, modalities=["rgb_static", "rel_actions_world"], train=True,
                                                 transform_manager=None, goal_strategy_prob=probs, goal_sampling_prob=P_GEOM,
                                                 nn_steps_from_step_path=str(d / "nn.json"), **HORIZON)
                if epoch is not None:
                    ds.increase_horizon(epoch)
                fid = lambda o: int(o["rgb_static"][0, 0, 0]) + 256 * int(o["rgb_static"][0, 0, 1])  # noqa: E731
                names = list(probs)
                codes = ["geometric", "similar_robot_obs", "random", "increasing_horizon", "episode_future", "next_state"]
                cols = {k: [] for k in ("idx", "step", "next", "goal", "reward", "done", "actions", "u_strategy", "disp", "u_choice",
                                        "strategy")}
                for idx in gen.randint(0, len(ds), size=ITEMS):
                    rec.clear()
                    it = ds[int(idx)]
                    draws = dict(rec)
                    assert len(draws) == len(rec) <= 2 and "u_strategy" in draws, rec  # at most one draw after the strategy's
                    assert fid(it["observations"]["goal"]) == fid(it["next_observations"]["goal"])
                    picked = names[int(np.searchsorted(np.cumsum(list(probs.values())), draws["u_strategy"], side="right").clip(0, len(names) - 1))]
                    for k, val in (("idx", int(idx)), ("step", fid(it["observations"]["observation"])),
                                   ("next", fid(it["next_observations"]["observation"])), ("goal", fid(it["observations"]["goal"])),
                                   ("reward", int(it["rewards"])), ("done", int(it["terminals"])), ("actions", np.asarray(it["actions"])),
                                   ("u_strategy", draws["u_strategy"]), ("disp", int(draws.get("disp", 1))),
                                   ("u_choice", draws.get("u_choice", 0.0)), ("strategy", codes.index(picked))):
                        cols[k].append(val)
                v = {k: np.asarray(c) for k, c in cols.items()}
                v["horizon"] = np.array(ds.current_horizon)
                v["len"] = np.array(len(ds))
                cov = coverage(variant, v, np.array(EP), {int(k): x for k, x in NN.items()})
                assert all(cov.values()), (variant, cov)
                print(variant, "len", len(ds), "horizon", ds.current_horizon, "covered:", ", ".join(cov))
                out.update({f"{variant}/{k}": a for k, a in v.items()})
        finally:
            np.random.choice, np.random.default_rng = o_choice, o_rng
        out["all_actions"] = acts
        out["ep"] = np.array(EP)
        out["nn"] = np.array(json.dumps(NN))
        out["cfg"] = np.array(json.dumps(dict(n_frames=N, goal_sampling_prob=P_GEOM, variants={k: [p, e] for k, (p, e) in VARIANTS.items()},
                                              **HORIZON)))
        path = os.path.join(ROOT, "tests", "golden", "transition_sampler.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path) / 1e3, "kB")


if __name__ == "__main__":
    main()
