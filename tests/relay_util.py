"""Shared by tests/test_relay_sampler_cpu.py and tests/test_relay_replay_gpu.py: the recorded items of the reference's
RILDataset (tests/golden/relay_sampler.npz, tools/gen_relay_golden.py)."""
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relay_sampler.npz")
ROLES = ("obs", "low_level_goal", "high_level_goal", "high_level_action")
KEYS = ("idx", "u_low", "u_high", "n_draws", "actions", "len") + ROLES
# the six (episodes, max_low_level_window, max_high_level_window) the fixture was recorded for
EXPECTED = [([[0, 69], [70, 159]], 30, 260), ([[0, 69], [70, 159]], 4, 12), ([[0, 39], [40, 52], [53, 99]], 1, 3),
            ([[0, 39], [40, 99]], 6, 6), ([[0, 39], [40, 99]], 8, 5), ([[0, 39], [40, 99]], 2, 1000)]


class RelayGolden:
    def __init__(self):
        G = np.load(PATH)
        self.cfg = json.loads(str(G["cfg"]))
        self.actions = G["all_actions"]
        self.settings = {k: (np.asarray(ep, dtype=np.int64), int(lw), int(hw)) for k, (ep, lw, hw) in self.cfg["variants"].items()}
        self.variants = {name: {k: G[f"{name}/{k}"] for k in KEYS} for name in self.settings}

    def n_frames(self, variant):
        return int(self.settings[variant][0].max()) + 1

    def index(self, variant, **kw):
        """The RelayIndex built with the settings the reference dataset of this variant was built with."""
        from tacorl_amd.data.relay_replay import RelayIndex

        ep, lw, hw = self.settings[variant]
        return RelayIndex(ep, n_frames=self.n_frames(variant), max_low_level_window=lw, max_high_level_window=hw, **kw)

    def draws(self, variant):
        """The recorded draws in RelayIndex.draw's form."""
        v = self.variants[variant]
        return {"idx": v["idx"].astype(np.int64), "u_low": v["u_low"].astype(np.float64), "u_high": v["u_high"].astype(np.float64)}

    def ids(self, variant):
        """The reference's four frame ids per item, (4, n) in ROLES order."""
        return np.stack([self.variants[variant][r] for r in ROLES]).astype(np.int64)


def extreme_draws(ix, n, seed):
    """n fresh draws whose first uniforms are the two extremes: 0.0 and the largest double below 1."""
    d = ix.draw(n, np.random.default_rng(seed))
    top = np.nextafter(1.0, 0.0)
    for k, vals in (("u_low", (0.0, top, 0.0, top)), ("u_high", (0.0, top, top, 0.0))):
        m = min(n, 4)
        d[k][:m] = vals[:m]
    return d
