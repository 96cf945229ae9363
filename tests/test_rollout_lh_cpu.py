"""The host side of the long-horizon rollout evaluation: the per-row restatement against the one already proven against the
kernel, the refill runner's schedule with a recording stub policy, and RolloutLongHorizon against
tests/golden/rollout_lh_callback.npz, which tools/gen_rollout_lh_callback_golden.py recorded from the reference's callback
with a scripted manager (the episodes are scripted here too: `_run_episodes` is the seam)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import rollout_envs as E
from tests import rollout_lh_envs as LH

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "rollout_lh_callback.npz")
MANAGER = {"_target_": "tacorl.evaluation.rollout_manager.TACORL", "plan_duration": 4}
WORLDS = [None, (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]
LENGTHS = [3, 9, 4, 17, 6, 1]


def _golden():
    with np.load(GOLDEN) as z:
        return {k.replace("__", "/"): json.loads(str(z[k])) for k in z.files}


# ------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("kind", ["normal", "uniform"])
@pytest.mark.parametrize("inner", [1, 3, 4, 5])
def test_rows_restatement_is_the_batch_restatement_on_consecutive_samples(kind, inner):
    from tacorl_amd import noise as N

    seed, step, did, B, sample0 = 0x0123_4567_89AB_CDEF, 7, N.DRAW_IDS["ro_plan"], 6, 5
    want = N.philox_restatement(seed, step, did, kind, B, inner, sample0=sample0)
    got = N.philox_rows_restatement(seed, did, kind, sample0 + np.arange(B), np.full(B, step), inner)
    assert got.shape == want.shape == (B, 1, inner) and got.dtype == want.dtype
    assert got.tobytes() == want.tobytes()
    other = N.philox_rows_restatement(seed, did, kind, sample0 + np.arange(B), np.full(B, step + 1), inner)
    assert not np.array_equal(other, got)


def test_rollout_draw_ids_are_appended():
    from tacorl_amd import noise as N

    assert [N.DRAW_IDS[k] for k in ("ro_rand_a", "ro_rand_b", "ro_plan", "ro_cem")] == [96, 97, 98, 99]
    assert N.DROPOUT_BASE + N.DROPOUT_MAX == 96 and list(N.DRAW_IDS)[-4:] == ["ro_rand_a", "ro_rand_b", "ro_plan", "ro_cem"]
    with pytest.raises(ValueError):
        N.rows_table(([0] * 65, [0] * 65, [0] * 65), [], 4)
    with pytest.raises(ValueError):
        N.rows_table(([0], [0], [0]), [N.RowSegment(0, "uniform", 96, 1)] * 5, 4)
    t = N.rows_table(([9, 9, 2], [1, 0, 5], [0, 0, 1]), [N.RowSegment(8, "normal", "ro_cem", 30, N.BY_PLAN, rows=[2, 0])], 128)
    assert (t.n_rows, t.n_seg, t.n_f32, t.seg[0].mask, t.seg[0].draw_id, t.seg[0].which) == (3, 1, 128, 0b101, 99, 1)
    assert list(t.episode[:3]) == [9, 9, 2] and list(t.step[:3]) == [1, 0, 5] and list(t.plan_no[:3]) == [0, 0, 1]


def test_the_entry_point_is_bound():
    from tacorl_amd import _lib

    assert "tacorl_noise_fill_rows" in _lib._SIGS and hasattr(_lib.lib(), "tacorl_noise_fill_rows")


# ------------------------------------------------------------------------------------------ the runner
class _StubPolicy:
    """A policy of R rows with LatentPlanPolicy's clock that records what the noise callable was given on every step."""

    def __init__(self, R, plan_duration=4):
        from tacorl_amd.evaluation.vec_policy import PlanClock

        self.R, self.clock, self.calls, self.resets = R, PlanClock(R, plan_duration), [], []

    def reset(self, rows=None):
        self.resets.append((len(self.calls), None if rows is None else list(rows)))
        self.clock.reset(rows)

    def step(self, observation, goal, noise=None):
        assert observation.shape[0] == self.R
        self.calls.append(noise["seen"])
        self.clock.tick(set(self.clock.due()))
        return torch.full((self.R, 8), float(len(self.calls)))


def _noise(keys, steps, due_rows):
    return {"seen": (list(keys), list(steps), list(due_rows))}


def _run(lengths, R, refill=True, **kw):
    from tacorl_amd.evaluation.vec_policy import rollout_episodes_refill

    pol, acts = _StubPolicy(R), []
    episodes = [(100 + i, {"length": n, "seed": i}) for i, n in enumerate(lengths)]
    infos = rollout_episodes_refill(pol, [LH.ScriptedVectorEnv() for _ in range(R)], episodes, noise=_noise, actions_out=acts,
                                    refill=refill, **kw)
    return pol, infos, acts


def test_refill_schedule():
    """Every episode sees its steps 0 .. len - 1 once and in order, its first step among the rows that re-plan; infos in episode
    order; a slot is refilled on the step after its episode ends; the policy is called as often as the greedy makespan says:
    slot 0 runs the episodes of 3, 4 and 17 steps back to back, 24 calls (the issue's text says 23; 3 + 4 + 17 is 24, and no
    schedule that keeps the queue's order can do with fewer)."""
    pol, infos, acts = _run(LENGTHS, 2)
    assert [i["episode_length"] for i in infos] == LENGTHS and [len(a) for a in acts] == LENGTHS
    seen = {}      # key -> [(call, row, step, due)]
    for c, (keys, steps, due) in enumerate(pol.calls):
        for r in range(2):
            seen.setdefault(keys[r], []).append((c, r, steps[r], r in due))
    ends = {}
    for i, n in enumerate(LENGTHS):
        rec = [x for x in seen[100 + i] if x[2] < n][:n]  # (an idle row repeats its last key with step == n)
        assert [x[2] for x in rec] == list(range(n)), (i, rec)
        assert [x[0] for x in rec] == list(range(rec[0][0], rec[0][0] + n))   # consecutive calls
        assert len({x[1] for x in rec}) == 1 and rec[0][3]                     # one slot; the first step re-plans
        assert [x[3] for x in rec] == [t % 4 == 0 for t in range(n)]           # ... and every plan_duration after it
        ends[i] = (rec[-1][0], rec[0][1], rec[0][0])
        # the episode's actions are the ones of its own calls (the stub answers call c with c + 1)
        assert [float(a[0]) for a in acts[i]] == [x[0] + 1.0 for x in rec]
    # refilled on the step after the end: episodes 2, 3 follow 0 and 2 in slot 0; 4, 5 follow 1 and 4 in slot 1
    for nxt, prev in ((2, 0), (3, 2), (4, 1), (5, 4)):
        assert ends[nxt][1] == ends[prev][1] and ends[nxt][2] == ends[prev][0] + 1, (nxt, prev, ends)
    assert len(pol.calls) == LH.greedy_makespan(LENGTHS, 2) == 24
    assert pol.resets[0] == (0, None) and [r for _, r in pol.resets[1:]] == [[0], [0], [1], [1]]
    for i in infos:
        assert set(i) == {"episode_length", "episode_return", "success", "successful_tasks"}


def test_fixed_batches_wait_for_their_slowest_row():
    pol, infos, acts = _run(LENGTHS, 2, refill=False)
    assert len(pol.calls) == LH.batch_makespan(LENGTHS, 2) == 9 + 17 + 6 == 32
    assert [i["episode_length"] for i in infos] == LENGTHS
    assert [r for _, r in pol.resets] == [None, [0, 1], [0, 1]] and [c for c, _ in pol.resets] == [0, 9, 26]
    ref, infos_r, _ = _run(LENGTHS, 2)
    assert len(ref.calls) <= len(pol.calls)
    for a, b in zip(infos, infos_r):  # the stub's actions differ with the call number, the lengths and keys do not
        assert a["episode_length"] == b["episode_length"]
    for lengths, R in (([5, 5, 5], 3), ([1, 2, 3, 4, 5, 6, 7], 3), ([7, 1, 1, 1, 7], 2), ([4], 1)):
        assert LH.greedy_makespan(lengths, R) <= LH.batch_makespan(lengths, R)
        assert len(_run(lengths, R)[0].calls) == LH.greedy_makespan(lengths, R)
        assert len(_run(lengths, R, refill=False)[0].calls) == LH.batch_makespan(lengths, R)


def test_spare_rows_idle_and_limits():
    pol, infos, acts = _run([3, 5], 4)
    assert len(pol.calls) == 5 and len(infos) == len(acts) == 2 and [len(a) for a in acts] == [3, 5]
    for keys, steps, due in pol.calls:
        assert keys[2:] == [None, None] and steps[2:] == [0, 0] and not set(due) & {2, 3}
    assert pol.calls[3][0][0] == 100 and pol.calls[3][1][0] == 3 and 0 not in pol.calls[4][2]  # the finished row idles
    # the step limit: max_steps and the environment's own
    pol, infos, _ = _run([9, 2, 9], 2, max_steps=4)
    assert [i["episode_length"] for i in infos] == [4, 2, 4] and len(pol.calls) == 6


def test_runner_refusals():
    from tacorl_amd.evaluation.vec_policy import rollout_episodes_refill

    envs = [LH.ScriptedVectorEnv() for _ in range(2)]
    with pytest.raises(ValueError, match="no episodes"):
        rollout_episodes_refill(_StubPolicy(2), envs, [])
    with pytest.raises(ValueError, match="policy of 3 rows"):
        rollout_episodes_refill(_StubPolicy(3), envs, [(0, {})])

    class Ingest:
        R = 3

    with pytest.raises(ValueError, match="ingest of 3 rows"):
        rollout_episodes_refill(_StubPolicy(2), envs, [(0, {})], ingest=Ingest())


# ------------------------------------------------------------------------------------------ the callback
class _Module:
    def __init__(self):
        self.current_epoch, self.logged, self.modes, self.saved = 0, [], [], 0

    def log(self, name, value, **kw):
        self.logged.append([name, float(value)])
        self.kw = kw

    def eval(self):
        self.modes.append("eval")

    def train(self):
        self.modes.append("train")

    def save_checkpoint(self):
        self.saved += 1


class _Env:
    _max_episode_steps = 0


@pytest.fixture(scope="module")
def state_dir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("rollout_lh_states"))
    E.write_state_dir(root, LH.START_END_TASKS)
    with open(os.path.join(root, "tasks.json"), "w") as f:
        json.dump(LH.START_END_TASKS, f)
    return root


def _callback(state_dir, k, **kw):
    from tacorl_amd.utils.callbacks.rollout_long_horizon import RolloutLongHorizon

    class Scripted(RolloutLongHorizon):
        """The episodes answered by scripted_info of what the callback asked for, as the golden's stub manager does."""

        def _run_episodes(self, pl_module, episodes):
            self.asked = getattr(self, "asked", [])
            self.keys = getattr(self, "keys", [])
            out = []
            for i, (g, reset_info) in enumerate(episodes):
                start, end, tasks = LH.key_of(reset_info)
                self.asked.append([start, end, tasks])
                self.keys.append(g)
                out.append(LH.scripted_info(start, end, tasks, i))
            return out

    kw.setdefault("envs", [_Env(), _Env()])
    return Scripted(num_rollouts=LH.NUM_ROLLOUTS, tasks_per_rollout=k, rollout_manager=MANAGER, data_dir=state_dir,
                    start_end_tasks=os.path.join(state_dir, "tasks.json"), max_episode_steps=33, **kw)


@pytest.mark.parametrize("k", [2, 4])
def test_task_list_as_the_reference_builds_it(state_dir, k):
    from tacorl_amd.utils.callbacks.rollout_long_horizon import get_long_horizon_tasks

    g = _golden()
    for sel in ("shortest", "as_listed"):
        cb = _callback(state_dir, k, val_every_n_epochs=1, id_selection_strategy=sel)
        assert cb.rollout_tasks == g[f"rollout_tasks/k{k}/{sel}"], sel
        assert get_long_horizon_tasks(LH.START_END_TASKS, k, sel) == cb.rollout_tasks
        assert cb.get_rollout_tasks(LH.START_END_TASKS, sel) == cb.rollout_tasks
    tasks = g[f"rollout_tasks/k{k}/shortest"]
    assert isinstance(tasks, list) and len(tasks) == {2: 5, 4: 4}[k] and all(len(w["completed_tasks"]) == k for w in tasks)
    assert [w["seq_len"] for w in tasks] == sorted(w["seq_len"] for w in tasks)
    if k == 4:  # windows of 70 .. 95 steps: there is no sequence-length filter
        assert min(w["seq_len"] for w in tasks) > E.MAX_SEQ_LEN
    assert cb.eval_strategy == "all_tasks" and (cb.num_rollouts, cb.tasks_per_rollout, cb.refill) == (7, k, True)


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("wr", WORLDS, ids=lambda w: "single" if w is None else f"world{w[0]}_rank{w[1]}")
def test_episodes_and_logs_are_the_reference_s(state_dir, monkeypatch, k, wr):
    """The episodes of the rank (window ids modulo the number of windows; the round-robin split), every logged name in order and
    every value; the draws' episode ids are the g of the split themselves."""
    import tacorl_amd.utils.callbacks.rollout as M
    import tacorl_amd.utils.callbacks.rollout_long_horizon as MLH

    g = _golden()
    tag = f"k{k}/" + ("single" if wr is None else f"world{wr[0]}_rank{wr[1]}")
    for mod in (M, MLH):
        monkeypatch.setattr(mod, "_world_rank", lambda: (None, 0) if wr is None else wr)
    cb, m = _callback(state_dir, k, val_every_n_epochs=1), _Module()
    cb.on_fit_start(None, m)
    val_info = cb.run_and_log_validation(m, on_step=False, on_epoch=True)
    assert cb.asked == g[f"asked/{tag}"]
    want = g[f"logged/{tag}"]
    assert [n for n, _ in m.logged] == [n for n, _ in want]
    assert [n for n, _ in want] == ["validation/LH_avg_episode_return", "validation/LH_avg_episode_length"] + \
        [f"validation/LH_{i + 1}_accuracy" for i in range(k)]
    for (n, v), (_, w) in zip(m.logged, want):
        assert v == pytest.approx(w, rel=1e-12, abs=0), n
    assert val_info == {n.split("/", 1)[1]: v for n, v in m.logged}
    assert m.kw["on_step"] is False and m.kw["on_epoch"] is True
    assert all(e._max_episode_steps == 33 for e in cb.envs) and m.modes == ["eval", "train"]
    assert cb.keys == M.rank_split(LH.NUM_ROLLOUTS, *(wr or (None, 0)))
    assert cb.last_infos is not None and len(cb.last_infos) == len(cb.keys)
    acc = [v for n, v in m.logged if n.endswith("_accuracy")]
    assert acc == sorted(acc, reverse=True)


def test_schedule_against_the_reference(state_dir):
    for case in _golden()["schedule"]:
        cb, m = _callback(state_dir, 2, **case["settings"]), _Module()
        cb.on_fit_start(None, m)
        rows = []
        for epoch in range(6):
            m.current_epoch = epoch
            n0, k0 = len(getattr(cb, "asked", [])), len(m.logged)
            cb.on_train_epoch_end(None, m)
            rows.append([epoch, len(getattr(cb, "asked", [])) > n0, sorted({n for n, _ in m.logged[k0:]})])
        assert rows == case["rows"], case["settings"]
        assert m.saved == 0 and not any(n.startswith("val_") for n, _ in m.logged)
        assert any(r[1] for r in rows)


def test_it_leaves_the_monitored_keys_and_the_checkpoint_to_the_rollout_entry(state_dir):
    from tacorl_amd import lightning as TL
    from tests.test_callbacks_rollout_cpu import _toy

    cb = _callback(state_dir, 2, val_every_n_epochs=1)
    mod = _toy(_Env())
    mod.saved = 0
    mod.save_checkpoint = lambda: setattr(mod, "saved", mod.saved + 1)
    tr = TL.MiniTrainer(max_epochs=2, callbacks=[cb])
    tr.fit(mod, [torch.zeros(1)] * 2)
    assert mod.saved == 0 and len(cb.asked) == 2 * LH.NUM_ROLLOUTS
    assert "val_accuracy" not in tr.logged_metrics and "val_episode_return" not in tr.logged_metrics
    assert {"validation/LH_1_accuracy", "validation/LH_2_accuracy", "validation/LH_avg_episode_return",
            "validation/LH_avg_episode_length"} <= set(tr.logged_metrics)


def test_an_empty_task_list_is_refused_by_name(state_dir):
    cb, m = _callback(state_dir, 5, val_every_n_epochs=1), _Module()
    assert cb.rollout_tasks == []
    cb.on_fit_start(None, m)
    with pytest.raises(ValueError, match=r"tasks_per_rollout = 5") as e:
        cb.run_and_log_validation(m, on_step=False, on_epoch=True)
    assert os.path.join(state_dir, "tasks.json") in str(e.value) and m.modes == ["eval", "train"]


def test_the_reference_target_builds_it(state_dir):
    from tacorl_amd.lightning import instantiate
    from tacorl_amd.utils.callbacks.rollout import Rollout
    from tacorl_amd.utils.callbacks.rollout_long_horizon import RolloutLongHorizon

    # config/callbacks/rollout_lh/default.yaml, the module path swapped as for every other callback
    cfg = {"_target_": "tacorl.utils.callbacks.rollout_long_horizon.RolloutLongHorizon".replace("tacorl.", "tacorl_amd.", 1),
           "_recursive_": False, "rollout_manager": MANAGER, "data_dir": state_dir,
           "start_end_tasks": os.path.join(state_dir, "tasks.json"), "val_every_n_epochs": 5, "num_rollouts": 32,
           "tasks_per_rollout": 2, "skip_first_n_epochs": 0, "max_episode_steps": 300, "min_seq_len": 32, "max_seq_len": 64}
    cb = instantiate(cfg, envs=[_Env()], refill=False, eval_strategy="episodes", log_video=True)
    assert type(cb) is RolloutLongHorizon and isinstance(cb, Rollout)
    assert (cb.num_rollouts, cb.tasks_per_rollout, cb.refill, cb.eval_strategy, cb.max_episode_steps) == (32, 2, False, "all_tasks", 300)
    assert len(cb.rollout_tasks) == 5
    d = RolloutLongHorizon(rollout_manager=MANAGER, data_dir=state_dir, start_end_tasks=os.path.join(state_dir, "tasks.json"),
                           val_every_n_epochs=1)
    assert (d.num_rollouts, d.tasks_per_rollout, d.refill) == (10, 4, True)
