"""Generate tests/golden/rollout_lh_callback.npz: what the UNMODIFIED reference long-horizon callback
(utils/callbacks/rollout_long_horizon.py RolloutLongHorizon) builds and logs - the task list of get_rollout_tasks for
tasks_per_rollout 2 and 4, and for each of them the episodes it asks its rollout manager for, as (window, tasks), and every
(name, value) it hands to `pl_module.log`, single rank and for every rank of a world of 2 and of 3 - recorded on CPU with a
stub manager that answers each episode with tests/rollout_lh_envs.py scripted_info, and the epochs on which
on_train_epoch_end evaluates for three val_every_n_epochs / skip_first_n_epochs settings (needs the reference checkout that
oracle/ref_harness.py points at).  num_rollouts is 7: divisible by neither world, larger than both task lists.

    python tools/gen_rollout_lh_callback_golden.py

The shims and the rank stand-in are tools/gen_rollout_callback_golden.py's.  The fixture holds names and numbers only, as JSON
strings."""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_rollout_callback_golden as G  # noqa: E402  (installs the shims on import)
from tests import rollout_envs as E  # noqa: E402
from tests import rollout_lh_envs as LH  # noqa: E402

from tacorl.utils.callbacks import rollout_long_horizon as R  # noqa: E402

SETTINGS = [dict(val_every_n_epochs=1), dict(val_every_n_epochs=2), dict(val_every_n_epochs=2, skip_first_n_epochs=3)]


class _Manager:
    """episode_rollout answers with scripted_info of what the callback asked for and the call's position."""

    def __init__(self):
        self.asked, self.tasks = [], []

    def episode_rollout(self, pl_module, env, reset_info=None, task=None, **kw):
        start, end, tasks = LH.key_of(reset_info)
        i = len(self.asked)
        self.asked.append([start, end, tasks])
        self.tasks.append(task)
        return LH.scripted_info(start, end, tasks, i)


def callback(tmp, k, **kw):
    cb = R.RolloutLongHorizon(num_rollouts=LH.NUM_ROLLOUTS, tasks_per_rollout=k, rollout_manager=_Manager(), data_dir=tmp,
                              start_end_tasks=os.path.join(tmp, "tasks.json"), max_episode_steps=33, **kw)
    cb.env, cb.video_logger, cb.transform_manager = G._Env(), G._Video(), None
    return cb


def main():
    out = {"num_rollouts": LH.NUM_ROLLOUTS}
    with tempfile.TemporaryDirectory() as tmp:
        E.write_state_dir(tmp, LH.START_END_TASKS)
        with open(os.path.join(tmp, "tasks.json"), "w") as f:
            json.dump(LH.START_END_TASKS, f)
        for k in (2, 4):
            for sel in ("shortest", "as_listed"):
                out[f"rollout_tasks/k{k}/{sel}"] = callback(tmp, k, val_every_n_epochs=1, id_selection_strategy=sel).rollout_tasks
            for wr in G.WORLDS:
                # (the subclass's module holds its own `dist` name; the base module's is not consulted by its evaluation)
                R.dist = G._Dist(wr)
                cb, m = callback(tmp, k, val_every_n_epochs=1), G._Module()
                assert cb.eval_strategy == "all_tasks"
                cb.run_and_log_validation(m, on_step=False, on_epoch=True)
                tag = f"k{k}/" + ("single" if wr is None else f"world{wr[0]}_rank{wr[1]}")
                out[f"asked/{tag}"] = cb.rollout_manager.asked
                out[f"logged/{tag}"] = m.logged
                assert cb.env._max_episode_steps == 33
                assert cb.rollout_manager.tasks == [f"long_horizon_{i + 1}" for i in range(len(cb.rollout_manager.asked))]
        R.dist = G._Dist(None)
        sched = []
        for s in SETTINGS:
            cb, m = callback(tmp, 2, **s), G._Module()
            rows = []
            for epoch in range(6):
                m.current_epoch = epoch
                n0, k0 = len(cb.rollout_manager.asked), len(m.logged)
                cb.on_train_epoch_end(None, m)
                rows.append([epoch, len(cb.rollout_manager.asked) > n0, sorted({n for n, _ in m.logged[k0:]})])
            sched.append({"settings": s, "rows": rows})
        out["schedule"] = sched
    path = os.path.join(ROOT, "tests", "golden", "rollout_lh_callback.npz")
    np.savez_compressed(path, **{k.replace("/", "__"): np.array(json.dumps(v)) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "entries")
    print(out["logged/k2/single"], out["asked/k4/world3_rank2"])


if __name__ == "__main__":
    main()
