"""Shared by tests/test_transition_sampler_cpu.py and tests/test_transition_replay_gpu.py: the recorded items of the
reference's GoalCondReplayBufferDataset (tests/golden/transition_sampler.npz, tools/gen_transition_golden.py)."""
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transition_sampler.npz")
KEYS = ("idx", "step", "next", "goal", "reward", "done", "actions", "u_strategy", "disp", "u_choice", "strategy", "horizon", "len")


class TransitionGolden:
    def __init__(self):
        G = np.load(PATH)
        self.cfg = json.loads(str(G["cfg"]))
        self.ep, self.actions = G["ep"], G["all_actions"]
        self.nn = {int(k): v for k, v in json.loads(str(G["nn"])).items()}
        self.variants = {name: {k: G[f"{name}/{k}"] for k in KEYS} for name in self.cfg["variants"]}

    def index(self, variant):
        """The TransitionIndex built with the settings the reference dataset of this variant was built with."""
        from tacorl_amd.data.replay import TransitionIndex

        probs, epoch = self.cfg["variants"][variant]
        ix = TransitionIndex(self.ep, n_frames=self.cfg["n_frames"], goal_strategy_prob=probs,
                             goal_sampling_prob=self.cfg["goal_sampling_prob"], initial_horizon=self.cfg["initial_horizon"],
                             horizon_step=self.cfg["horizon_step"], max_horizon=self.cfg["max_horizon"], nn_steps_from_step=self.nn)
        if epoch is not None:
            ix.increase_horizon(epoch)
        return ix

    def draws(self, variant, ix):
        """The recorded draws in TransitionIndex.draw's form (the strategy from the recorded uniform, as the index maps it)."""
        v = self.variants[variant]
        return {"idx": v["idx"].astype(np.int64), "strategy": ix.strategy_of(v["u_strategy"]), "disp": v["disp"].astype(np.int64),
                "u_choice": v["u_choice"].astype(np.float64)}


def coverage(variant, v, ep, nn):
    """What a variant's recorded items must include, where the variant's strategies can produce it at all: reward 0 and 1
    (next_state: only 1; random: 1 is a 1-in-56 event, not required), a goal clipped by the episode end (geometric: the draw
    reached past the end; increasing_horizon: the horizon did), an empty neighbour list that took the random fallback, and
    random picks on both sides of the removed step (possible_steps is sorted: a pick below / above it = a goal below / above)."""
    step, goal, rew = v["step"], v["goal"], v["reward"]
    end = ep[np.searchsorted(ep[:, 0], step, side="right") - 1, 1]
    out = {}
    if variant != "next_state":
        out["reward 0"] = bool((rew == 0).any())
    if variant != "random":
        out["reward 1"] = bool((rew == 1).any())
    if variant in ("geo_sim", "horizon", "horizon_epoch3"):
        far = v["disp"] > end - step if variant == "geo_sim" else v["horizon"] > end - step
        out["clipped by the episode end"] = bool((far & (goal == end) & (v["strategy"] != 1)).any())
    if variant == "horizon":
        out["horizon inside the episode"] = bool((v["horizon"] < end - step).any())
    if variant in ("geo_sim", "random"):
        empty = np.array([len(nn[int(s)]) == 0 for s in step])
        fb = empty & (v["strategy"] == 1) if variant == "geo_sim" else np.ones(len(step), bool)
        out["random fallback"] = bool(fb.any())
        out["random pick below the removed step"] = bool((fb & (goal < step)).any())
        out["random pick above the removed step"] = bool((fb & (goal > step)).any())
        if variant == "geo_sim":
            out["a neighbour pick"] = bool(((v["strategy"] == 1) & ~fb).any())
    return out
