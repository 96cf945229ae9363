"""The rollout evaluation that ends every experiment's callback group (reference utils/callbacks/rollout.py; config/callbacks/
{play_lmp,tacorl,offline_rl_goal_cond,relay_imitation_learning}.yaml -> `rollout:`): every `val_every_n_*` the module is
rolled out in its environments and `val_accuracy` / `val_episode_return` - what the `checkpoint: accuracy` group monitors -
are logged.

    Rollout(rollout_manager={"_target_": "tacorl.evaluation.rollout_manager.TACORL", "plan_duration": 16},
            val_every_n_epochs=1, eval_strategy="all_tasks", data_dir=..., start_end_tasks=..., envs=[env0, env1, ...])

The schedule, the task list, the three strategies, the split of the episodes over ranks and every logged key are the
reference's (line numbers of utils/callbacks/rollout.py in the comments).  What differs is how the episodes run: the
reference's managers roll ONE episode at a time; here the strategy's episodes are listed first and run R = len(envs) at a
time through evaluation/vec_policy.py rollout_episodes - episodes of different tasks share a batch, finished rows idle.  The
`_target_` leaf of `rollout_manager` selects the policy: RLRollout -> RLPolicy, LatentPlanRollout / TACORL -> LatentPlanPolicy,
RelayImitationLearning -> RelayPolicy; image modules are fed through FrameIngest from the environments' raw uint8 frames.
Every draw an episode consumes (the sampled plan of LatentPlanRollout, the action decoder's mixture draws, CEM's population)
comes from a generator keyed by (seed, episode, purpose, number), so an episode's trajectory does not depend on R, on the row
it runs in or on the rank split, and the evaluation leaves torch's generators - and with them the training run - alone.

`envs`: a list of gym-API environments, or a callable i -> environment together with `n_envs`; None: `pl_module.env` alone.
Metrics logged with sync_dist=True in the reference are averaged over ranks here (dist.reduce_logs_), and the monitored
`val_*` keys are computed from the averaged values, so every rank's checkpoint callback sees the same number.

The `rollout_lh:` entry of the same callback groups is rollout_long_horizon.py RolloutLongHorizon, a subclass of Rollout
whose episodes run through a refilled queue with device-drawn noise.
Not built: video logging, `render` and wandb - `log_video` is accepted and ignored."""
import hashlib
import json
import logging
import math
import os

import numpy as np
import torch

from ... import dist as _D
from ...lightning import CallbackBase

log = logging.getLogger(__name__)

IMAGE_MANAGERS = ("RLRollout", "LatentPlanRollout", "TACORL", "RelayImitationLearning")


# ------------------------------------------------------------------------------------------ pure parts
def rank_split(n, world=None, rank=0):
    """The episodes of one rank (:160-167, :294-303, :409-413): all n without a process group; otherwise the
    g < world * ceil(n / world) with g % world == rank - every rank runs the same number, some g reach past n."""
    if world is None:
        return list(range(n))
    return [g for g in range(world * math.ceil(n / world)) if g % world == rank]


def _world_rank():
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(), dist.get_rank()
    return None, 0


def get_rollout_tasks(start_end_tasks, id_selection_strategy="shortest", min_seq_len=16, max_seq_len=64):
    """:101-126.  Windows that complete exactly one task, max_seq_len > seq_len > min_seq_len; a task whose windows are all
    outside keeps an empty list (and is skipped by evaluate_all_tasks)."""
    rollout_tasks = {}
    for start_idx, end_tasks in start_end_tasks.items():
        for end_idx, completed_tasks in end_tasks.items():
            if len(completed_tasks) == 1:
                task = completed_tasks[0]
                rollout_tasks.setdefault(task, [])
                seq_len = int(end_idx) - int(start_idx)
                if max_seq_len > seq_len > min_seq_len:
                    rollout_tasks[task].append({"start_step": int(start_idx), "end_step": int(end_idx), "seq_len": seq_len})
    if id_selection_strategy == "shortest":
        for key, value in rollout_tasks.items():
            rollout_tasks[key] = sorted(value, key=lambda d: d["seq_len"])
    return rollout_tasks


def _mean(xs):
    return float(np.mean(xs))


def grouped_metrics(per_task):
    """The aggregation of evaluate_all_tasks / evaluate_env_tasks (:193-259, :316-385).  per_task: [(task, infos)] in
    evaluation order, infos the task's rollout_info dicts (one per entry of its goal list).  Returns (logs, val_info): logs
    the [(suffix, {metric: value})] published as `<log_type>/<suffix>/<metric>` - per task, then "dynamic" ("block" in the
    task's name), then "static" - and val_info the mean of the two groups."""
    groups = {k: {"episode_returns": [], "episodes_lengths": [], "succesful_episodes": 0, "total_episodes": 0}
              for k in ("dynamic", "static")}
    logs = []
    for task, infos in per_task:
        returns = [i["episode_return"] for i in infos]
        lengths = [i["episode_length"] for i in infos]
        wins = sum(int(i["success"]) for i in infos)
        g = groups["dynamic" if "block" in task else "static"]
        g["episode_returns"].extend(returns)
        g["episodes_lengths"].extend(lengths)
        g["succesful_episodes"] += wins
        g["total_episodes"] += len(infos)
        logs.append((task, {"accuracy": wins / len(infos), "avg_episode_return": _mean(returns), "avg_episode_length": _mean(lengths)}))
    out = {}
    for name in ("dynamic", "static"):
        g = groups[name]
        if g["total_episodes"] == 0:
            # :219-221, :232-234 divide by total_episodes: the reference ends in a ZeroDivisionError here
            raise ValueError(f"no episode of the evaluation falls into the {name} group ('block' "
                             f"{'in' if name == 'dynamic' else 'not in'} the task's name): its accuracy is 0 / 0")
        out[name] = {"accuracy": g["succesful_episodes"] / g["total_episodes"],
                     "avg_episode_return": _mean(g["episode_returns"]), "avg_episode_length": _mean(g["episodes_lengths"])}
        logs.append((name, out[name]))
    val_info = {k: (out["dynamic"][k] + out["static"][k]) / 2 for k in ("accuracy", "avg_episode_return", "avg_episode_length")}
    return logs, val_info


def flat_metrics(infos, score=False):
    """`evaluate` (:427-431; rollout_d4rl.py:88-93)."""
    wins = sum(int(i["success"]) for i in infos)
    out = {"accuracy": wins / len(infos), "avg_episode_return": _mean([i["episode_return"] for i in infos]),
           # :430 takes the mean of the success COUNT (np.mean(val_info["succesful_episodes"])), not of the lengths: copied
           "avg_episode_length": _mean(wins)}
    if score:
        out["score"] = _mean([i["score"] for i in infos])
    return out


def keyed_generator(seed, episode, purpose, number):
    """A host generator that depends on (seed, episode, purpose, number) and on nothing else."""
    h = hashlib.blake2b(f"{int(seed)}/{episode}/{purpose}/{int(number)}".encode(), digest_size=8).digest()
    return torch.Generator().manual_seed(int.from_bytes(h, "little") >> 1)


def manager_leaf(rollout_manager):
    """(class name, is it a D4RL manager, its remaining settings) of a rollout-manager config."""
    cfg = dict(rollout_manager or {})
    target = str(cfg.pop("_target_", ""))
    for k in ("_recursive_", "_convert_"):
        cfg.pop(k, None)
    leaf = target.rsplit(".", 1)[-1]
    d4rl = "d4rl" in target.rsplit(".", 1)[0]
    known = ("RLRollout", "LatentPlanRollout", "TACORL") if d4rl else IMAGE_MANAGERS
    if leaf not in known:
        raise ValueError(f"rollout_manager._target_ {target!r}: one of {', '.join(known)} of "
                         f"tacorl.evaluation.{'rollout_manager_d4rl' if d4rl else 'rollout_manager'} is built")
    return leaf, d4rl, cfg


# ------------------------------------------------------------------------------------------ the callback
class RolloutBase(CallbackBase):
    """What utils/callbacks/rollout.py and rollout_d4rl.py share: the schedule, the environments, the batched episode runner."""

    SCORE = False  # the D4RL callback also publishes the normalised score

    def _init_schedule(self, rollout_manager, val_episodes, skip_first_n_epochs, val_every_n_epochs, val_every_n_episodes,
                       val_every_n_batches, envs, n_envs, seed):
        assert (val_every_n_epochs is not None or val_every_n_episodes is not None
                or val_every_n_batches is not None), "val_every_n ... is not set"  # :53-57
        self.val_every_n_episodes, self.val_every_n_epochs = val_every_n_episodes, val_every_n_epochs
        self.val_every_n_batches, self.val_episodes = val_every_n_batches, val_episodes
        self.skip_first_n_epochs = skip_first_n_epochs
        self.rollout_manager = rollout_manager
        self.manager, self.d4rl, self.manager_cfg = manager_leaf(rollout_manager)
        self.seed = int(seed)
        if callable(envs):
            if n_envs is None or int(n_envs) < 1:
                raise ValueError("envs is a callable i -> environment: give n_envs, how many to build")
            envs = [envs(i) for i in range(int(n_envs))]
        elif envs is not None:
            envs = list(envs)
            if not envs:
                raise ValueError("envs is empty")
            if n_envs is not None and int(n_envs) != len(envs):
                raise ValueError(f"n_envs {n_envs} for a list of {len(envs)} environments")
        self.envs = envs
        self._policies, self._ingests = {}, {}
        self.last_infos = None  # the rollout_info dicts of the last evaluation, in episode order
        self.last_actions = None

    # ------------------------------------------------------------------ environments and policies
    def on_fit_start(self, trainer, pl_module) -> None:
        """:485-496."""
        if self.envs is None:
            env = getattr(pl_module, "env", None)
            if env is None:
                raise ValueError(f"{type(self).__name__}: no environment - {type(pl_module).__name__}.env is None. Pass the "
                                 "environments to the callback: envs=[env0, env1, ...] (gym-API objects, one episode runs in "
                                 "each at a time) or envs=lambda i: make_env(i) with n_envs=R")
            self.envs = [env]
        self.env = self.envs[0]
        if not hasattr(self, "transform_manager"):
            dm = getattr(trainer, "datamodule", None)
            self.transform_manager = (self.manager_cfg.get("transform_manager") or getattr(dm, "transform_manager", None)
                                      or getattr(pl_module, "transform_manager", None) or None)

    def _policy(self, pl_module, R):
        """(policy, ingest or None) of R rows for this module, built once per R."""
        if R not in self._policies:
            from ...evaluation.vec_policy import LatentPlanPolicy, RelayPolicy, RLPolicy

            cfg, dur = self.manager_cfg, int(self.manager_cfg.get("plan_duration", 16))
            if self.manager == "RLRollout":
                pol = RLPolicy(pl_module, R, use_cem=bool(cfg.get("use_cem", False)))
            elif self.manager == "RelayImitationLearning":
                pol = RelayPolicy(pl_module, R, plan_duration=dur)
            else:
                pol = LatentPlanPolicy(pl_module, R, plan_duration=dur,
                                       use_cem=self.manager == "TACORL" and bool(cfg.get("use_cem", False)))
            ingest = None
            if not self.d4rl:
                from ...evaluation.frame_ingest import FrameIngest

                ingest = FrameIngest(pl_module, R, self.transform_manager, use_cem=getattr(pol, "cem", None) is not None)
            self._policies[R], self._ingests[R] = pol, ingest
        return self._policies[R], self._ingests[R]

    def _noise(self, pol, keys):
        """step -> the noise dict of a batch whose row r runs episode keys[r]."""
        ad, cem = getattr(pol, "ad", None), getattr(pol, "cem", None)
        dur = getattr(pol, "plan_duration", 1)
        if ad is None and cem is None:
            return None
        samples_plan = ad is not None and getattr(pol, "actor", None) is None

        def at(t):
            out = {}
            if ad is not None:
                gs = [keyed_generator(self.seed, k, "decoder", t) for k in keys]
                out["rand_a"] = torch.stack([torch.rand(ad.Da, ad.K, generator=g) for g in gs])
                out["rand_b"] = torch.stack([torch.rand(ad.Da, generator=g) for g in gs])
            if t % dur == 0:  # the step on which every row of the batch re-plans (all episodes began at step 0)
                if samples_plan:
                    out["plan_eps"] = torch.stack([torch.randn(ad.P, generator=keyed_generator(self.seed, k, "plan", t // dur))
                                                   for k in keys])
                if cem is not None:
                    shape = (cem.num_iterations, cem.batch_size, cem.action_dim)
                    out["cem_eps"] = torch.stack([torch.randn(*shape, generator=keyed_generator(self.seed, k, "cem", t // dur))
                                                  for k in keys])
            return out

        return at

    def _run_episodes(self, pl_module, episodes):
        """episodes: [(key, reset_info)] -> their rollout_info dicts in the same order, R = len(self.envs) at a time."""
        from ...evaluation.vec_policy import rollout_episodes

        infos, R = [], len(self.envs)
        self.last_actions = []  # per episode, the actions its environment was stepped with
        dev = getattr(pl_module, "dev", None)
        cuda = [dev] if dev is not None and torch.device(dev).type == "cuda" else []
        with torch.no_grad(), torch.random.fork_rng(devices=cuda):
            for i in range(0, len(episodes), R):
                part = episodes[i: i + R]
                pol, ingest = self._policy(pl_module, len(part))
                envs = self.envs[: len(part)]
                acts = []
                got = rollout_episodes(pol, envs, noise=self._noise(pol, [k for k, _ in part]),
                                       reset_infos=[ri for _, ri in part], ingest=ingest, actions_out=acts)
                self.last_actions += acts
                if self.SCORE:
                    for env, info in zip(envs, got):
                        info["score"] = env.get_normalized_score(info["episode_return"])  # rollout_manager_d4rl.py:98
                infos += got
        return infos

    # ------------------------------------------------------------------ logging
    def _log_metrics(self, pl_module, entries, on_step, on_epoch):
        """pl_log_metrics(..., sync_dist=True) for [(name, value)]: one collective over all of them (dist.reduce_logs_)."""
        if not entries:
            return []
        vals = torch.tensor([float(v) for _, v in entries], dtype=torch.float64)
        world, _ = _world_rank()
        if world is not None and _D.group_ready() and _D.collectives_on(world):
            import torch.distributed as dist

            t = vals.to(pl_module.dev) if dist.get_backend() == "nccl" else vals  # (fp64: one rank's sum is the value itself)
            t, div = _D.reduce_logs_(t, world)
            vals = t.to("cpu") / div
        out = [(name, float(v)) for (name, _), v in zip(entries, vals)]
        for name, v in out:
            pl_module.log(name, v, on_step=on_step, on_epoch=on_epoch, sync_dist=True)
        return out

    def _evaluate_and_log(self, pl_module, log_type, on_step, on_epoch):
        raise NotImplementedError

    def run_and_log_validation(self, pl_module, log_type="validation", on_step=True, on_epoch=True):
        """:436-483."""
        for env in self.envs:
            if hasattr(self, "max_episode_steps"):
                env._max_episode_steps = self.max_episode_steps  # :443
        pl_module.eval()
        try:
            val_info = self._evaluate_and_log(pl_module, log_type, on_step, on_epoch)
        finally:
            pl_module.train()
        if "accuracy" in val_info and "avg_episode_return" in val_info:
            log.info("Validation | Accuracy: %.2f, Return: %.2f", val_info["accuracy"], val_info["avg_episode_return"])
        reduced = self._log_metrics(pl_module, [(f"{log_type}/{k}", v) for k, v in val_info.items()], on_step, on_epoch)
        return {name.split("/", 1)[1]: v for name, v in reduced}

    # ------------------------------------------------------------------ schedule
    def on_train_batch_end(self, trainer, pl_module, outputs, batch, batch_idx, unused=0) -> None:
        """:498-515."""
        if (pl_module.current_epoch >= self.skip_first_n_epochs and self.val_every_n_batches is not None
                and batch_idx % self.val_every_n_batches == 0):
            self.run_and_log_validation(pl_module, log_type="batch_val")

    def on_train_epoch_end(self, trainer, pl_module) -> None:
        """:517-547."""
        val_info = {"avg_episode_return": float("-inf"), "accuracy": float("-inf"), "score": float("-inf")}
        if pl_module.current_epoch >= self.skip_first_n_epochs:
            episode_cond = (self.val_every_n_episodes is not None and hasattr(pl_module, "episode_number")
                            and pl_module.episode_number.item() % self.val_every_n_episodes == 0
                            and hasattr(pl_module, "episode_done") and pl_module.episode_done)
            epoch_cond = self.val_every_n_epochs is not None and pl_module.current_epoch % self.val_every_n_epochs == 0
            if episode_cond or epoch_cond:
                val_info = self.run_and_log_validation(pl_module, on_step=False, on_epoch=True)
                if hasattr(pl_module, "save_checkpoint"):
                    pl_module.save_checkpoint()
        # monitored metric to save top k model
        pl_module.log("val_episode_return", val_info["avg_episode_return"], on_epoch=True)
        pl_module.log("val_accuracy", val_info["accuracy"], on_epoch=True)
        if self.SCORE:
            pl_module.log("val_score", val_info["score"], on_epoch=True)


class Rollout(RolloutBase):
    """reference utils/callbacks/rollout.py Rollout, with `envs` / `n_envs` / `seed` added (see the module's docstring).
    `log_video` is accepted and ignored: video logging, `render` and wandb are not built."""

    def __init__(self, rollout_manager, val_episodes=5, max_episode_steps=100, skip_first_n_epochs=0, val_every_n_epochs=None,
                 val_every_n_episodes=None, val_every_n_batches=None, eval_strategy="all_tasks",
                 data_dir="~/tacorl/calvin/validation", start_end_tasks="~/tacorl/calvin/start_end_tasks.json",
                 id_selection_strategy="shortest", num_rollouts_per_task=3, min_seq_len=16, max_seq_len=64, envs=None,
                 n_envs=None, seed=0, log_video=False):
        self._init_schedule(rollout_manager, val_episodes, skip_first_n_epochs, val_every_n_epochs, val_every_n_episodes,
                            val_every_n_batches, envs, n_envs, seed)
        self.eval_strategy, self.max_episode_steps = eval_strategy, max_episode_steps
        if self.eval_strategy == "all_tasks":  # :67-83
            self.num_rollouts_per_task, self.min_seq_len, self.max_seq_len = num_rollouts_per_task, min_seq_len, max_seq_len
            from ...data.frame_dir import step_files

            self.data_dir = os.path.expanduser(str(data_dir))
            assert os.path.isdir(self.data_dir), f"{self.data_dir} not found"
            self.step_to_file = step_files(self.data_dir)
            path = os.path.expanduser(str(start_end_tasks))
            assert os.path.isfile(path), f"{path} not found"
            with open(path) as f:
                self.rollout_tasks = get_rollout_tasks(json.load(f), id_selection_strategy, min_seq_len, max_seq_len)

    def get_state_info_from_step(self, step):
        """:94-99."""
        with np.load(self.step_to_file(step), allow_pickle=True) as state:
            return {"robot_obs": state["robot_obs"], "scene_obs": state["scene_obs"]}

    # ------------------------------------------------------------------ the three strategies
    def all_tasks_episodes(self, world=None, rank=0):
        """[(task, [(key, reset_info)])] of evaluate_all_tasks (:149-183) for one rank."""
        out = []
        for ti, (task, windows) in enumerate(self.rollout_tasks.items()):
            if len(windows) == 0:  # :157
                continue
            eps = []
            for g in rank_split(self.num_rollouts_per_task, world, rank):
                w = windows[g % len(windows)]  # :170 "make sure goal list is valid"
                eps.append(((ti, g), {"task_info": {"start_info": self.get_state_info_from_step(w["start_step"]),
                                                    "goal_info": self.get_state_info_from_step(w["end_step"]),
                                                    "tasks": [task]}}))
            out.append((task, eps))
        return out

    def env_tasks_episodes(self, possible_tasks, world=None, rank=0):
        """The same of evaluate_env_tasks (:284-306)."""
        out = []
        for ti, (task, num_goals) in enumerate(possible_tasks.items()):
            eps = [((ti, g), {"task_info": {"task": task, "index": g % num_goals}}) for g in rank_split(num_goals, world, rank)]
            out.append((task, eps))
        return out

    def _grouped(self, pl_module, per_task_eps, log_type, on_step, on_epoch):
        flat = [e for _, eps in per_task_eps for e in eps]
        infos = self._run_episodes(pl_module, flat)
        self.last_infos = infos
        per_task, i = [], 0
        for task, eps in per_task_eps:
            per_task.append((task, infos[i: i + len(eps)]))
            i += len(eps)
        logs, val_info = grouped_metrics(per_task)
        self._log_metrics(pl_module, [(f"{log_type}/{suffix}/{k}", v) for suffix, m in logs for k, v in m.items()], on_step, on_epoch)
        return val_info

    def evaluate_all_tasks(self, pl_module, render=False, log_type="validation", on_step=False, on_epoch=True):
        world, rank = _world_rank()
        return self._grouped(pl_module, self.all_tasks_episodes(world, rank), log_type, on_step, on_epoch)

    def evaluate_env_tasks(self, pl_module, render=False, log_type="validation", on_step=False, on_epoch=True):
        world, rank = _world_rank()
        return self._grouped(pl_module, self.env_tasks_episodes(self.env.get_possible_tasks(), world, rank), log_type, on_step,
                             on_epoch)

    def evaluate(self, pl_module, num_episodes=5, render=False, device="cuda"):
        world, rank = _world_rank()
        infos = self._run_episodes(pl_module, [(("episode", e), {}) for e in rank_split(num_episodes, world, rank)])
        self.last_infos = infos
        return flat_metrics(infos, score=self.SCORE)

    def _evaluate_and_log(self, pl_module, log_type, on_step, on_epoch):
        if self.eval_strategy == "all_tasks":  # :445-464
            return self.evaluate_all_tasks(pl_module, log_type=log_type, on_step=on_step, on_epoch=on_epoch)
        if self.eval_strategy == "env_tasks" and hasattr(self.env, "get_possible_tasks"):
            return self.evaluate_env_tasks(pl_module, log_type=log_type, on_step=on_step, on_epoch=on_epoch)
        return self.evaluate(pl_module, num_episodes=self.val_episodes)
