"""Generate tests/golden/nn_table.npz: the nn_steps_from_step file that the UNMODIFIED reference GoalCondReplayBufferDataset
writes (set_nn_steps_from_step, datamodule/dataset/goal_cond_replay_buffer_dataset.py:76-130) for a tiny synthetic dataset
in a temp dir whose per-frame files carry `robot_obs` and which has NO nn.json, so that the class takes its own build path
(needs the reference checkout that oracle/ref_harness.py points at).

    python tools/gen_nn_table_golden.py

faiss is no dependency of this project and need not be installed.  A stand-in module named `faiss` is put into sys.modules; its IndexFlatL2(d).add / .search is
the search as this project defines it (include/tacorl_hip.h tacorl_knn_l2: fp32 direct-form distances, (distance, row)
order), computed by tacorl_amd.data.neighbours.knn_l2_host.

What the fixture pins: the reference's own post-processing - which frames are searched (range(start, end) per episode, the
end steps left out), the margin rule (applied after the top-k, |dt| < 16 dropped, == 16 kept, across episodes), the order of
the surviving lists and the file schema ({"train": {"<step>": [...]}}, indent=4).
What it does not pin: real faiss.  Its tie order and the rounding of its BLAS-expanded distances are not reproduced, so a
table built by real faiss can differ from this one on ties and near-ties only.

The fixture holds the points, the episodes, num_nn, margin and the JSON text the reference wrote.  No reference source text."""
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
from tacorl_amd.data.neighbours import knn_l2_host  # noqa: E402

H.install_shims()
_core = types.ModuleType("hydra.core")
_hc = types.ModuleType("hydra.core.hydra_config")
_hc.HydraConfig = type("HydraConfig", (), {})
_core.hydra_config = _hc
sys.modules["hydra.core"], sys.modules["hydra.core.hydra_config"] = _core, _hc
sys.modules["hydra"].core = _core
sys.modules["hydra.utils"].get_original_cwd = os.getcwd
from tacorl.datamodule.dataset.goal_cond_replay_buffer_dataset import GoalCondReplayBufferDataset  # noqa: E402

EP = [[0, 120], [121, 199], [200, 299]]  # three episodes of unequal length
N, D, NUM_NN = 300, 15, 8
MARGIN = 16  # the reference's default: set_nn_steps_from_step is called with num_nn only
DUPLICATES = [(250, 10), (60, 140), (290, 30)]  # (copy, original): exact duplicate frames far apart in time


def robot_obs():
    """Smooth periodic trajectories: episode 0 repeats every 15 steps with a small drift (neighbours at |dt| = 15 inside the
    margin, at 30 and 45 outside), episode 1 every 40 steps, episode 2 is a slow one-way motion (only temporal neighbours:
    empty lists)."""
    rs = np.random.RandomState(0)
    t = np.arange(N, dtype=np.float64)[:, None]
    phase, amp = rs.uniform(0, 2 * np.pi, D)[None, :], rs.uniform(0.2, 1.0, D)[None, :]
    x = np.zeros((N, D))
    a, b, c = (slice(s, e + 1) for s, e in EP)
    x[a] = amp * np.sin(2 * np.pi * t[a] / 15 + phase) + 2e-3 * t[a]
    x[b] = 1.5 + amp * np.sin(2 * np.pi * t[b] / 40 + phase) + 1e-3 * t[b]
    x[c] = -2.0 + 0.05 * amp * (t[c] - 200)
    x = x.astype(np.float32)
    for dst, src in DUPLICATES:
        x[dst] = x[src]
    return x


class _IndexFlatL2:
    def __init__(self, d):
        self.d, self.x = d, None

    def add(self, x):
        assert x.dtype == np.float32 and x.shape[1] == self.d
        self.x = x if self.x is None else np.concatenate([self.x, x])

    def search(self, q, k):
        assert q is self.x or np.array_equal(q, self.x)  # the reference searches the table against itself
        rows, dist = knn_l2_host(self.x, k)
        return dist, rows.astype(np.int64)


def coverage(nn, pts, ep, num_nn, margin):
    """What the fixture must include (tests/test_nn_table_cpu.py asserts the same)."""
    steps = np.concatenate([np.arange(s, e) for s, e in ep])
    rows, _ = knn_l2_host(pts[steps], num_nn)
    dt = np.abs(steps[rows] - steps[:, None])
    return {"keys are the range(start, end) steps": sorted(nn) == steps.tolist(),
            "an empty list": any(len(v) == 0 for v in nn.values()),
            "a list with survivors": any(len(v) > 0 for v in nn.values()),
            "a neighbour dropped at |dt| = margin - 1": bool((dt == margin - 1).any()),
            "a neighbour kept at |dt| >= margin": bool((dt >= margin).any())}


def main():
    obs = robot_obs()
    fake = types.ModuleType("faiss")
    fake.IndexFlatL2 = _IndexFlatL2
    sys.modules["faiss"] = fake
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        for i in range(N):
            np.savez(d / f"episode_{i:07d}.npz", rgb_static=np.zeros((2, 2, 3), np.uint8), rel_actions_world=np.zeros(7, np.float32),
                     robot_obs=obs[i])
        np.save(d / "ep_start_end_ids.npy", np.array(EP))
        assert not (d / "nn.json").exists()
        ds = GoalCondReplayBufferDataset(data_dir=d, modalities=["rgb_static", "rel_actions_world"], train=True,
                                         transform_manager=None, goal_strategy_prob={"geometric": 0.5, "similar_robot_obs": 0.5},
                                         nn_steps_from_step_path=str(d / "nn.json"), num_nn=NUM_NN)
        text = (d / "nn.json").read_text()
    doc = json.loads(text)
    assert list(doc) == ["train"] and {int(k): v for k, v in doc["train"].items()} == dict(ds.nn_steps_from_step)
    nn = {int(k): v for k, v in doc["train"].items()}
    cov = coverage(nn, obs, np.array(EP), NUM_NN, MARGIN)
    assert all(cov.values()), cov
    lens = [len(v) for v in nn.values()]
    print(f"{len(nn)} steps, list lengths {min(lens)}..{max(lens)}, {sum(n == 0 for n in lens)} empty; covered:", ", ".join(cov))
    path = os.path.join(ROOT, "tests", "golden", "nn_table.npz")
    np.savez_compressed(path, robot_obs=obs, ep=np.array(EP), num_nn=np.array(NUM_NN), margin=np.array(MARGIN),
                        nn_json=np.array(text))
    print("wrote", path, os.path.getsize(path) / 1e3, "kB")


if __name__ == "__main__":
    main()
