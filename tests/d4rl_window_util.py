"""Shared by tools/gen_d4rl_window_golden.py, tests/test_d4rl_window_sampler_cpu.py and tests/test_d4rl_replay_gpu.py: the
recorded items of the reference's D4RLPlayDataset (tests/golden/d4rl_window_sampler.npz), the synthetic dataset they were
recorded on, and what a variant's items must include."""
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "d4rl_window_sampler.npz")
KEYS = ("idx", "window", "disp", "observations", "actions", "goal", "goal_reached", "len", "ep")
DATASET_KEYS = ("observations", "actions", "timeouts", "terminals")
EPISODE_LENGTHS = (40, 9, 25, 1, 60, 17)  # + TRAILING frames behind the last end, which belong to no episode
TRAILING = 5
BOTH_FLAGS_AT = 2  # the end of this episode has `timeouts` and `terminals` set
# variant -> D4RLPlayDataset / D4RLWindowIndex settings
VARIANTS = {
    "lmp_8_16": dict(min_window_size=8, max_window_size=16, include_goal=False),
    "tacorl_8_8": dict(min_window_size=8, max_window_size=8, include_goal=True, goal_sampling_prob=0.3),
    "tacorl_8_16": dict(min_window_size=8, max_window_size=16, include_goal=True, goal_sampling_prob=0.3),
    "tacorl_thr": dict(min_window_size=8, max_window_size=16, include_goal=True, goal_sampling_prob=0.6, goal_threshold=0.3),
}


def grid_walk(rs, n, lo=0.0, hi=16.0, step=1.0 / 16):
    """(n, 2) positions: a +-step random walk on the `step` grid inside [lo, hi).  With step = 1/16 and hi = 16 every
    coordinate difference is a multiple of 1/16 below 16, so dx*dx + dy*dy has at most 17 significant bits: it is exact in
    fp32 with or without FMA contraction, and `sqrt(d2) < threshold` cannot depend on a rounding."""
    pos = np.empty((n, 2), dtype=np.float64)
    p = np.array([rs.randint(0, int((hi - lo) / step)) * step + lo for _ in range(2)])
    for i in range(n):
        pos[i] = p
        p = np.clip(p + rs.choice([-step, step], size=2), lo, hi - step)
    return pos.astype(np.float32)


def synthetic_dataset(lengths=EPISODE_LENGTHS, trailing=TRAILING, S=29, A=8, seed=0, both_at=BOTH_FLAGS_AT):
    """The four D4RL arrays: episodes of `lengths` whose ends alternate between `timeouts` and `terminals` (one end has both
    set), `trailing` frames behind the last end; observation columns 0-1 a grid walk, the rest uniform noise."""
    rs = np.random.RandomState(seed)
    n = int(sum(lengths)) + trailing
    obs = rs.uniform(-1, 1, size=(n, S)).astype(np.float32)
    obs[:, :2] = grid_walk(rs, n)
    act = rs.uniform(-1, 1, size=(n, A)).astype(np.float32)
    timeouts, terminals = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for k, e in enumerate(np.cumsum(lengths) - 1):
        (timeouts if k % 2 == 0 else terminals)[e] = True
        if k == both_at:
            timeouts[e] = terminals[e] = True
    return {"observations": obs, "actions": act, "timeouts": timeouts, "terminals": terminals}


def coverage(variant, v, ep, cfg):
    """What a variant's recorded items must include: both values of goal_reached, a goal clipped by the episode end and one
    that is not, disp == 1 (the goal is the window's last row), window == min, == max and one in between where the window
    varies, and an item of the one-item episode (the last one)."""
    idx, ws, disp = v["idx"], v["window"], v["disp"]
    mx, mn = cfg["max_window_size"], cfg["min_window_size"]
    lookup = np.concatenate([np.arange(s, max(e + 1 - mx, s)) for s, e in ep])
    s = lookup[idx]
    end = ep[np.searchsorted(ep[:, 0], s, side="right") - 1, 1]
    out = {}
    if ep[-1, 1] + 1 - mx - ep[-1, 0] == 1:  # (with max = 16 the last episode, 17 frames, has one item)
        out["an item of the one-item episode"] = bool((s == ep[-1, 0]).any())
    if mn != mx:
        out.update({"window == min": bool((ws == mn).any()), "window == max": bool((ws == mx).any()),
                    "a window in between": bool(((ws > mn) & (ws < mx)).any())})
    if cfg.get("include_goal"):
        far = s + (ws - 1) * disp > end
        out.update({"goal_reached False": bool((~v["goal_reached"]).any()), "goal_reached True": bool(v["goal_reached"].any()),
                    "goal clipped by the episode end": bool(far.any()), "goal inside the episode": bool((~far).any()),
                    "disp == 1": bool((disp == 1).any())})
    return out


class D4rlWindowGolden:
    def __init__(self):
        G = np.load(PATH)
        self.cfg = json.loads(str(G["cfg"]))
        self.dataset = {k: G[f"dataset/{k}"] for k in DATASET_KEYS}
        self.variants = {name: {k: G[f"{name}/{k}"] for k in KEYS} for name in self.cfg["variants"]}

    def index(self, variant):
        """The D4RLWindowIndex built with the settings the reference dataset of this variant was built with."""
        from tacorl_amd.data.d4rl_replay import D4RLWindowIndex

        return D4RLWindowIndex(self.dataset["timeouts"], self.dataset["terminals"], **self.cfg["variants"][variant])

    def draws(self, variant):
        v = self.variants[variant]
        return {k: v[k].astype(np.int64) for k in ("idx", "window", "disp")}
