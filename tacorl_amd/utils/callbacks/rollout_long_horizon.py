"""The long-horizon evaluation of the simulator experiments (reference utils/callbacks/rollout_long_horizon.py; config/callbacks/
{play_lmp,tacorl,offline_rl_goal_cond,relay_imitation_learning}.yaml -> `rollout_lh:`): `num_rollouts` episodes, each reset to
the start of a window of start_end_tasks.json that completes exactly `tasks_per_rollout` tasks, and the share of episodes that
completed at least 1, 2, ... of them - `validation/LH_{i}_accuracy`, the paper's headline number.

    RolloutLongHorizon(rollout_manager={"_target_": "tacorl.evaluation.rollout_manager.TACORL", "plan_duration": 16},
                       num_rollouts=32, tasks_per_rollout=2, max_episode_steps=300, val_every_n_epochs=5, data_dir=...,
                       start_end_tasks=..., envs=[env0, env1, ...])

The task list, the split of the episodes over ranks, the metrics and the schedule are the reference's (its line numbers in the
comments).  What differs is how the episodes run.  They end when their last task succeeds, anywhere between a few steps and
`max_episode_steps`, so they go through evaluation/vec_policy.py rollout_episodes_refill: a queue over the R = len(envs)
slots in which a slot takes the next episode the step after its own ends (refill=False: fixed batches of R that wait for
their slowest row - the same episodes, for comparison).  Rows are then at different steps of different episodes, so every
step's draws come from ONE tacorl_noise_fill_rows launch (noise.py RowNoise) keyed per row by (seed, episode g, step or plan
number): nothing is drawn or uploaded by the host, and an episode's trajectory does not depend on R, on its slot, on the
refill or on the rank split.  Torch's generators are left alone.

It publishes `validation/LH_*` only: `val_accuracy` / `val_episode_return` and `save_checkpoint` belong to the sibling
`rollout:` entry.  `log_video` and `render` are accepted and ignored."""
import json
import os

import numpy as np
import torch

from .rollout import Rollout, _world_rank, rank_split


# ------------------------------------------------------------------------------------------ pure parts
def get_long_horizon_tasks(start_end_tasks, tasks_per_rollout, id_selection_strategy="shortest"):
    """:30-48.  The windows that complete exactly tasks_per_rollout tasks, as a list; no sequence-length filter."""
    rollout_tasks = []
    for start_idx, end_tasks in start_end_tasks.items():
        for end_idx, completed_tasks in end_tasks.items():
            if len(completed_tasks) == tasks_per_rollout:
                rollout_tasks.append({"start_step": int(start_idx), "end_step": int(end_idx),
                                      "seq_len": int(end_idx) - int(start_idx), "completed_tasks": completed_tasks})
    if id_selection_strategy == "shortest":
        rollout_tasks = sorted(rollout_tasks, key=lambda d: d["seq_len"])
    return rollout_tasks


def long_horizon_metrics(infos, tasks_per_rollout):
    """:103-117.  LH_{i}_accuracy: the episodes with at least i successful tasks over the episodes of this rank."""
    done = np.zeros(tasks_per_rollout, dtype=np.int64)
    for i in infos:
        done[: len(i["successful_tasks"])] += 1
    out = {"LH_avg_episode_return": float(np.mean([i["episode_return"] for i in infos])),
           "LH_avg_episode_length": float(np.mean([i["episode_length"] for i in infos]))}
    for k in range(tasks_per_rollout):
        out[f"LH_{k + 1}_accuracy"] = float(done[k] / len(infos))
    return out


def row_noise(pol, seed):
    """(keys, steps, due_rows) -> the step's noise dict for `pol.step`, as rollout_episodes_refill asks for it: views of ONE
    device buffer carved here, filled by one tacorl_noise_fill_rows launch per step.  keys are the episodes' integer ids.
    rand_a (R, Da, K) and rand_b (R, Da) are uniforms numbered by the row's step, drawn for every row; plan_eps (R, P) - where
    the plan is sampled - and cem_eps (R, iters, N, P) are normals numbered by step // plan_duration, drawn for due_rows only
    (the other rows keep what they held: the policy does not read them).  None for a policy that draws nothing."""
    from ... import noise as N

    R = pol.R
    ad, cem = getattr(pol, "ad", None), getattr(pol, "cem", None)
    dur = int(getattr(pol, "plan_duration", 1))
    carve = []  # (name in policy.step's noise dict, draw, kind, shape per row, numbered by, drawn for every row)
    if ad is not None:
        carve += [("rand_a", "ro_rand_a", "uniform", (ad.Da, ad.K), N.BY_STEP, True),
                  ("rand_b", "ro_rand_b", "uniform", (ad.Da,), N.BY_STEP, True)]
        if getattr(pol, "actor", None) is None:
            carve.append(("plan_eps", "ro_plan", "normal", (ad.P,), N.BY_PLAN, False))
    if cem is not None:
        carve.append(("cem_eps", "ro_cem", "normal", (cem.num_iterations, cem.batch_size, cem.action_dim), N.BY_PLAN, False))
    if not carve:
        return None
    offs, total = [], 0
    for c in carve:
        offs.append(total)
        total = (total + R * int(np.prod(c[3])) + 3) // 4 * 4
    buf = torch.zeros(total, device=pol.dev)
    views = {c[0]: buf[o: o + R * int(np.prod(c[3]))].view(R, *c[3]) for c, o in zip(carve, offs)}
    gen = N.RowNoise(int(seed) % (1 << 64))

    def at(keys, steps, due_rows):
        segs = [N.RowSegment(o, kind, draw, int(np.prod(shape)), which, rows=None if every else due_rows)
                for (_, draw, kind, shape, which, every), o in zip(carve, offs)]
        gen.fill(([0 if k is None else int(k) for k in keys], steps, [s // dur for s in steps]), segs, buf)
        return views

    return at


class RolloutLongHorizon(Rollout):
    """reference RolloutLongHorizon with Rollout's `envs` / `n_envs` / `seed` and `refill` added (see the module's docstring)."""

    def __init__(self, num_rollouts=10, tasks_per_rollout=4, *args, refill=True, **kwargs):
        self.num_rollouts, self.tasks_per_rollout, self.refill = int(num_rollouts), int(tasks_per_rollout), bool(refill)
        kwargs["eval_strategy"] = "all_tasks"  # :27
        super().__init__(*args, **kwargs)
        self.start_end_tasks = os.path.expanduser(str(kwargs.get("start_end_tasks", "~/tacorl/calvin/start_end_tasks.json")))
        with open(self.start_end_tasks) as f:
            self.rollout_tasks = get_long_horizon_tasks(json.load(f), self.tasks_per_rollout,
                                                        kwargs.get("id_selection_strategy", "shortest"))
        self._row_noises = {}

    def get_rollout_tasks(self, start_end_tasks, id_selection_strategy="shortest"):
        return get_long_horizon_tasks(start_end_tasks, self.tasks_per_rollout, id_selection_strategy)

    # ------------------------------------------------------------------ the episodes
    def long_horizon_episodes(self, world=None, rank=0):
        """[(g, reset_info)] of one rank (:70-93): episode g runs window g modulo the number of windows; g itself keys its draws."""
        if len(self.rollout_tasks) == 0:  # (:59-60 returns None, and run_and_log_validation fails on `"accuracy" in None`)
            raise ValueError(f"no window of {self.start_end_tasks} completes exactly tasks_per_rollout = "
                             f"{self.tasks_per_rollout} tasks: there is nothing to roll out")
        out = []
        for g in rank_split(self.num_rollouts, world, rank):
            w = self.rollout_tasks[g % len(self.rollout_tasks)]  # :80 "make sure rollout_list is valid"
            out.append((g, {"task_info": {"start_info": self.get_state_info_from_step(w["start_step"]),
                                          "goal_info": self.get_state_info_from_step(w["end_step"]),
                                          "tasks": w["completed_tasks"]}}))
        return out

    def _row_noise(self, pol):
        if pol.R not in self._row_noises:
            self._row_noises[pol.R] = row_noise(pol, self.seed)
        return self._row_noises[pol.R]

    def _run_episodes(self, pl_module, episodes):
        """episodes: [(g, reset_info)] -> their rollout_info dicts in the same order, through the len(self.envs) slots."""
        from ...evaluation.vec_policy import rollout_episodes_refill

        pol, ingest = self._policy(pl_module, len(self.envs))
        dev = getattr(pl_module, "dev", None)
        cuda = [dev] if dev is not None and torch.device(dev).type == "cuda" else []
        acts = []
        with torch.no_grad(), torch.random.fork_rng(devices=cuda):
            infos = rollout_episodes_refill(pol, self.envs, episodes, noise=self._row_noise(pol), ingest=ingest,
                                            actions_out=acts, refill=self.refill)
        self.last_actions = acts
        return infos

    def evaluate_all_tasks(self, pl_module, render=False, log_type="validation", on_step=False, on_epoch=True):
        """:50-120."""
        world, rank = _world_rank()
        infos = self._run_episodes(pl_module, self.long_horizon_episodes(world, rank))
        self.last_infos = infos
        return long_horizon_metrics(infos, self.tasks_per_rollout)

    # ------------------------------------------------------------------ schedule
    def on_train_epoch_end(self, trainer, pl_module) -> None:
        """:122-132.  The epoch condition alone; no val_* keys, no checkpoint."""
        if (pl_module.current_epoch >= self.skip_first_n_epochs and self.val_every_n_epochs is not None
                and pl_module.current_epoch % self.val_every_n_epochs == 0):
            self.run_and_log_validation(pl_module, on_step=False, on_epoch=True)
