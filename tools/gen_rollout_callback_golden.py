"""Generate tests/golden/rollout_callback.npz: what the UNMODIFIED reference rollout callback (utils/callbacks/rollout.py
Rollout) builds and logs - the task list of get_rollout_tasks, and for evaluate_all_tasks / evaluate_env_tasks / evaluate
the episodes it asks its rollout manager for and every (name, value) it hands to `pl_module.log`, single rank and for every
rank of a world of 2 and of 3 - recorded on CPU with a stub manager that answers each episode with
tests/rollout_envs.py scripted_info(key), and the epochs / batches on which on_train_epoch_end / on_train_batch_end evaluate
for a list of val_every_n_* / skip_first_n_epochs settings (needs the reference checkout that oracle/ref_harness.py points
at).

    python tools/gen_rollout_callback_golden.py

The rank split is evaluated as a pure function: the callback module's `dist` name is pointed at a stand-in that reports
(world, rank); no process group exists.  The fixture holds names and numbers only, as JSON strings."""
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as H  # noqa: E402
from tests import rollout_envs as E  # noqa: E402

H.install_shims()


class _Callback:
    """pl.Callback's hooks the reference callback passes on to (`super().on_train_epoch_end(...)`)."""

    def on_fit_start(self, *a, **k):
        pass

    def on_train_batch_end(self, *a, **k):
        pass

    def on_train_epoch_end(self, *a, **k):
        pass


sys.modules["pytorch_lightning"].Callback = _Callback
# shims of this tool alone: the callback module's imports that the harness does not cover
hc = types.ModuleType("hydra.core")
hcc = types.ModuleType("hydra.core.hydra_config")
hcc.HydraConfig = type("HydraConfig", (), {"initialized": staticmethod(lambda: False)})
sys.modules["hydra.core"], sys.modules["hydra.core.hydra_config"] = hc, hcc
sys.modules["hydra.utils"].get_original_cwd = os.getcwd
for name in ("wandb", "wandb.util"):
    sys.modules.setdefault(name, types.ModuleType(name))
cv2 = sys.modules["cv2"]
for name in ("INTER_AREA", "INTER_LINEAR"):
    if not hasattr(cv2, name):
        setattr(cv2, name, 0)
from tacorl.utils.callbacks import rollout as R  # noqa: E402

NUM_ROLLOUTS, VAL_EPISODES = 3, 5
WORLDS = [None, (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]


class _Dist:
    def __init__(self, wr):
        self.wr = wr

    def is_available(self):
        return self.wr is not None

    def is_initialized(self):
        return self.wr is not None

    def get_world_size(self):
        return self.wr[0]

    def get_rank(self):
        return self.wr[1]


class _Module:
    def __init__(self):
        self.current_epoch, self.logged = 0, []

    def log(self, name, value, **kw):
        self.logged.append([name, float(value)])

    def eval(self):
        pass

    def train(self):
        pass


class _Manager:
    """episode_rollout answers with scripted_info of what the callback asked for."""

    def __init__(self):
        self.asked, self.count = [], 0

    def episode_rollout(self, pl_module, env, reset_info=None, **kw):
        if reset_info is None:
            key = ("episode", self.count)
        else:
            ti = reset_info["task_info"]
            if "start_info" in ti:
                key = (ti["tasks"][0], int(ti["start_info"]["robot_obs"][2]), int(ti["goal_info"]["robot_obs"][2]))
            else:
                key = (ti["task"], int(ti["index"]))
        self.count += 1
        self.asked.append(list(key))
        return E.scripted_info(*key)


class _Env:
    _max_episode_steps = 0

    def get_possible_tasks(self):
        return dict(E.TASKS)


class _Video:
    def log(self, *a, **k):
        pass


def callback(tmp, strategy, **kw):
    cb = R.Rollout(rollout_manager=_Manager(), eval_strategy=strategy, data_dir=tmp, start_end_tasks=os.path.join(tmp, "tasks.json"),
                   num_rollouts_per_task=NUM_ROLLOUTS, min_seq_len=E.MIN_SEQ_LEN, max_seq_len=E.MAX_SEQ_LEN,
                   val_episodes=VAL_EPISODES, max_episode_steps=33, **kw)
    cb.env, cb.video_logger, cb.transform_manager = _Env(), _Video(), None
    return cb


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        E.write_state_dir(tmp)
        with open(os.path.join(tmp, "tasks.json"), "w") as f:
            json.dump(E.START_END_TASKS, f)
        for sel in ("shortest", "as_listed"):
            cb = callback(tmp, "all_tasks", val_every_n_epochs=1, id_selection_strategy=sel)
            out[f"rollout_tasks/{sel}"] = cb.rollout_tasks
        for strategy in ("all_tasks", "env_tasks", "episodes"):
            for wr in WORLDS:
                R.dist = _Dist(wr)
                cb, m = callback(tmp, strategy, val_every_n_epochs=1), _Module()
                val_info = cb.run_and_log_validation(m, on_step=False, on_epoch=True)
                tag = f"{strategy}/" + ("single" if wr is None else f"world{wr[0]}_rank{wr[1]}")
                out[f"asked/{tag}"] = cb.rollout_manager.asked
                out[f"logged/{tag}"] = m.logged
                out[f"val_info/{tag}"] = {k: float(v) for k, v in val_info.items()}
                assert cb.env._max_episode_steps == 33
        R.dist = _Dist(None)
        # the schedule: which epochs (of 6) and which batches (of 4 per epoch) evaluate, and what the epoch publishes
        settings = [dict(val_every_n_epochs=1), dict(val_every_n_epochs=2), dict(val_every_n_epochs=2, skip_first_n_epochs=3),
                    dict(val_every_n_batches=2), dict(val_every_n_batches=3, skip_first_n_epochs=1),
                    dict(val_every_n_epochs=3, val_every_n_batches=4), dict(val_every_n_episodes=1)]
        sched = []
        for s in settings:
            cb, m = callback(tmp, "episodes", **s), _Module()
            rows = []
            for epoch in range(6):
                m.current_epoch = epoch
                for b in range(4):
                    n0 = cb.rollout_manager.count
                    cb.on_train_batch_end(None, m, None, None, b)
                    rows.append(["batch", epoch, b, cb.rollout_manager.count > n0])
                n0, k0 = cb.rollout_manager.count, len(m.logged)
                cb.on_train_epoch_end(None, m)
                pub = dict((n, v) for n, v in m.logged[k0:] if n in ("val_accuracy", "val_episode_return"))
                rows.append(["epoch", epoch, -1, cb.rollout_manager.count > n0, pub["val_accuracy"], pub["val_episode_return"]])
            sched.append({"settings": s, "rows": rows})
        out["schedule"] = sched
    try:
        R.Rollout(rollout_manager=None)
        raise SystemExit("the reference accepted a callback without val_every_n_*")
    except AssertionError as e:
        out["no_schedule_message"] = str(e)
    path = os.path.join(ROOT, "tests", "golden", "rollout_callback.npz")
    enc = lambda v: np.array(json.dumps(v).replace("-Infinity", '"-inf"'))  # noqa: E731
    np.savez_compressed(path, **{k.replace("/", "__"): enc(v) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "entries")
    print(out["logged/all_tasks/single"][-6:], out["val_info/all_tasks/single"])


if __name__ == "__main__":
    main()
