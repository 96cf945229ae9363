"""Generate tests/golden/d4rl_window_sampler.npz: what the UNMODIFIED reference D4RLPlayDataset.__getitem__
(datamodule/dataset/d4rl_play_dataset.py:69-146) returns on a small synthetic dataset, with every numpy draw it consumes
recorded (needs the reference checkout that oracle/ref_harness.py points at).

    python tools/gen_d4rl_window_golden.py

The fixture holds the four dataset arrays (tests/d4rl_window_util.py synthetic_dataset: about 160 frames in episodes of
40, 9, 25, 1, 60 and 17 frames plus 5 trailing ones), and per variant and item: the item index, the recorded draws (the
window size of np.random.randint, the displacement of default_rng().geometric), the returned observations, actions, goal
and goal_reached - plus the reference's ep_start_end_ids and len.  No reference source text.
Beside oracle.ref_harness's stand-ins this adds an empty `d4rl` module and a `gym.make` whose result has `get_dataset()`."""
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as H  # noqa: E402
from tests.d4rl_window_util import PATH, VARIANTS, coverage, synthetic_dataset  # noqa: E402

ITEMS = 64
SEED = 3  # (every coverage condition holds, and no recorded distance equals a threshold: 0.5 is a point of the 1/16 grid)
DATA = synthetic_dataset()

H.install_shims()
sys.modules.setdefault("d4rl", types.ModuleType("d4rl"))
sys.modules["gym"].make = lambda name, *a, **k: types.SimpleNamespace(get_dataset=lambda: DATA)
from tacorl.datamodule.dataset.d4rl_play_dataset import D4RLPlayDataset  # noqa: E402
from tacorl.utils.transforms import TransformManager  # noqa: E402


def main():
    snapshot = {k: v.copy() for k, v in DATA.items()}
    gen = np.random.RandomState(SEED)
    rec = []
    o_randint, o_rng = np.random.randint, np.random.default_rng

    def randint(low, high=None, *a, **kw):
        v = int(gen.randint(low, high))
        rec.append(("window", v))
        return v

    class FakeRng:
        def geometric(self, p):
            v = int(gen.geometric(p))
            rec.append(("disp", v))
            return v

    out = {f"dataset/{k}": v for k, v in DATA.items()}
    np.random.randint, np.random.default_rng = randint, lambda *a, **k: FakeRng()
    try:
        for variant, cfg in VARIANTS.items():
            # the `rl` transform manager names no transform for observations / actions: they only become float tensors
            ds = D4RLPlayDataset(transform_manager=TransformManager({"train": {}, "validation": {}}), transf_type="train",
                                 pad=True, **cfg)
            ep = np.asarray(ds.ep_start_end_ids, dtype=np.int64)
            cols = {k: [] for k in ("idx", "window", "disp", "observations", "actions", "goal", "goal_reached")}
            items = gen.randint(0, len(ds), size=ITEMS)
            items[0] = len(ds) - 1  # the last item: with max = 16 the one item of the 17-frame episode
            for idx in items:
                rec.clear()
                it = ds[int(idx)]
                draws = dict(rec)
                assert len(draws) == len(rec) and set(draws) <= {"window", "disp"}, rec
                assert ("window" in draws) == (cfg["min_window_size"] != cfg["max_window_size"])
                assert ("disp" in draws) == cfg["include_goal"] == ("goal" in it)
                assert it["idx"] == idx and it["window_size"] == draws.get("window", cfg["max_window_size"])
                assert it["observations"].dtype == it["actions"].dtype and str(it["observations"].dtype) == "torch.float32"
                goal = np.asarray(it["goal"]) if "goal" in it else np.zeros(2, np.float32)
                assert goal.dtype == np.float32
                if "goal" in it:
                    assert isinstance(it["goal_reached"], (bool, np.bool_)), type(it["goal_reached"])
                    s = ds.episode_lookup[int(idx)]
                    d = float(np.linalg.norm(goal.astype(np.float64) - DATA["observations"][s + it["window_size"] - 1][:2]))
                    thr = cfg.get("goal_threshold", 0.5)
                    assert abs(d - thr) > 1e-6 * thr, (variant, idx, d)  # no recorded distance on the threshold
                for k, val in (("idx", int(idx)), ("window", int(it["window_size"])), ("disp", int(draws.get("disp", 1))),
                               ("observations", it["observations"].numpy()), ("actions", it["actions"].numpy()), ("goal", goal),
                               ("goal_reached", bool(it.get("goal_reached", False)))):
                    cols[k].append(val)
            v = {k: np.asarray(c) for k, c in cols.items()}
            v["len"], v["ep"] = np.array(len(ds)), ep
            cov = coverage(variant, v, ep, cfg)
            assert all(cov.values()), (variant, cov)
            print(variant, "len", len(ds), "episodes", ep.tolist(), "reached", int(v["goal_reached"].sum()), "of", ITEMS,
                  "windows", sorted(set(v["window"].tolist())), "covered:", ", ".join(cov))
            out.update({f"{variant}/{k}": a for k, a in v.items()})
    finally:
        np.random.randint, np.random.default_rng = o_randint, o_rng
    assert all(np.array_equal(snapshot[k], DATA[k]) for k in DATA), "the reference wrote into the dataset"
    out["cfg"] = np.array(json.dumps(dict(items=ITEMS, seed=SEED, variants=VARIANTS)))
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH) / 1e3, "kB")


if __name__ == "__main__":
    main()
