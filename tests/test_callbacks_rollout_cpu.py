"""The rollout callback's host side against tests/golden/rollout_callback.npz, which tools/gen_rollout_callback_golden.py recorded
from the reference's Rollout with a scripted manager: the task list, the id selection with its modulo wrap, the split of the
episodes over ranks, every logged (name, value) of the three strategies, the schedule through MiniTrainer, and the refusals.
The episodes themselves are scripted here too (tests/rollout_envs.py scripted_info): `_run_episodes` is the seam."""
import json
import os

import numpy as np
import pytest
import torch

from tests import rollout_envs as E

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "rollout_callback.npz")
MANAGER = {"_target_": "tacorl.evaluation.rollout_manager.TACORL", "plan_duration": 4}
WORLDS = [None, (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]


def _golden():
    with np.load(GOLDEN) as z:
        out = {k.replace("__", "/"): json.loads(str(z[k])) for k in z.files}
    return out


def _unwrap(v):
    return float("-inf") if v == "-inf" else v


def _scripted(cls):
    class Scripted(cls):
        """The episodes answered by scripted_info of what the callback asked for, as the golden's stub manager does."""

        def _run_episodes(self, pl_module, episodes):
            self.asked = getattr(self, "asked", [])
            out = []
            for _, reset_info in episodes:
                if not reset_info:
                    key = ("episode", len(self.asked))  # (the stub manager counts its calls, across evaluations)
                else:
                    ti = reset_info["task_info"]
                    key = ((ti["tasks"][0], int(ti["start_info"]["robot_obs"][2]), int(ti["goal_info"]["robot_obs"][2]))
                           if "start_info" in ti else (ti["task"], int(ti["index"])))
                self.asked.append(list(key))
                info = E.scripted_info(*key)
                if self.SCORE:
                    info["score"] = 2.0 * info["episode_return"]
                out.append(info)
            return out

    return Scripted


class _Module:
    def __init__(self, env=None):
        self.current_epoch, self.logged, self.env, self.modes = 0, [], env, []

    def log(self, name, value, **kw):
        self.logged.append([name, float(value)])

    def eval(self):
        self.modes.append("eval")

    def train(self):
        self.modes.append("train")


class _Env:
    _max_episode_steps = 0

    def get_possible_tasks(self):
        return dict(E.TASKS)


@pytest.fixture(scope="module")
def state_dir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("rollout_states"))
    E.write_state_dir(root)
    with open(os.path.join(root, "tasks.json"), "w") as f:
        json.dump(E.START_END_TASKS, f)
    return root


def _callback(state_dir, strategy, **kw):
    from tacorl_amd.utils.callbacks.rollout import Rollout

    kw.setdefault("envs", [_Env(), _Env()])
    return _scripted(Rollout)(rollout_manager=MANAGER, eval_strategy=strategy, data_dir=state_dir,
                              start_end_tasks=os.path.join(state_dir, "tasks.json"), num_rollouts_per_task=3,
                              min_seq_len=E.MIN_SEQ_LEN, max_seq_len=E.MAX_SEQ_LEN, val_episodes=5, max_episode_steps=33, **kw)


def test_task_list_as_the_reference_builds_it(state_dir):
    g = _golden()
    for sel in ("shortest", "as_listed"):
        cb = _callback(state_dir, "all_tasks", val_every_n_epochs=1, id_selection_strategy=sel)
        assert cb.rollout_tasks == g[f"rollout_tasks/{sel}"], sel
        assert list(cb.rollout_tasks) == list(g[f"rollout_tasks/{sel}"])  # evaluation order
    tasks = g["rollout_tasks/shortest"]
    assert all(E.MAX_SEQ_LEN > w["seq_len"] > E.MIN_SEQ_LEN for ws in tasks.values() for w in ws)
    assert [w["seq_len"] for w in tasks["open_drawer"]] == [20, 20, 40] and len(tasks["move_block_left"]) == 2
    info = cb.get_state_info_from_step(263)
    assert np.array_equal(info["robot_obs"], E.state_of_step(263)["robot_obs"]) and sorted(info) == ["robot_obs", "scene_obs"]


@pytest.mark.parametrize("strategy", ["all_tasks", "env_tasks", "episodes"])
@pytest.mark.parametrize("wr", WORLDS, ids=lambda w: "single" if w is None else f"world{w[0]}_rank{w[1]}")
def test_strategies_log_what_the_reference_logs(state_dir, monkeypatch, strategy, wr):
    """Episodes asked for (ids modulo the number of candidates; the round-robin split), every logged name in order and
    every value, the returned val_info and env._max_episode_steps."""
    import tacorl_amd.utils.callbacks.rollout as M

    g = _golden()
    tag = f"{strategy}/" + ("single" if wr is None else f"world{wr[0]}_rank{wr[1]}")
    monkeypatch.setattr(M, "_world_rank", lambda: (None, 0) if wr is None else wr)
    cb, m = _callback(state_dir, strategy, val_every_n_epochs=1), _Module()
    cb.on_fit_start(None, m)
    val_info = cb.run_and_log_validation(m, on_step=False, on_epoch=True)
    assert cb.asked == g[f"asked/{tag}"]
    want = g[f"logged/{tag}"]
    assert [n for n, _ in m.logged] == [n for n, _ in want]
    for (n, v), (_, w) in zip(m.logged, want):
        assert v == pytest.approx(w, rel=1e-12, abs=0), n
    assert val_info == pytest.approx(g[f"val_info/{tag}"], rel=1e-12)
    assert all(e._max_episode_steps == 33 for e in cb.envs) and m.modes == ["eval", "train"]


def test_rank_split_is_the_reference_round_robin():
    from tacorl_amd.utils.callbacks.rollout import rank_split

    assert rank_split(3) == [0, 1, 2]
    assert [rank_split(3, 2, r) for r in range(2)] == [[0, 2], [1, 3]]
    assert [rank_split(5, 3, r) for r in range(3)] == [[0, 3], [1, 4], [2, 5]]
    assert rank_split(4, 1, 0) == [0, 1, 2, 3]


def test_the_reference_oddity_of_evaluate_is_copied():
    """avg_episode_length of `evaluate` is the mean of the success COUNT (:430)."""
    from tacorl_amd.utils.callbacks.rollout import flat_metrics

    infos = [dict(episode_length=7, episode_return=-1.0, success=True), dict(episode_length=9, episode_return=-3.0, success=True),
             dict(episode_length=4, episode_return=-2.0, success=False)]
    assert flat_metrics(infos) == {"accuracy": 2 / 3, "avg_episode_return": -2.0, "avg_episode_length": 2.0}


# ------------------------------------------------------------------------------------------ schedule through MiniTrainer
def _toy(env=None):
    from tacorl_amd import lightning as TL

    class Toy(TL.LightningModuleBase):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))
            self.automatic_optimization = False
            self.env = env

        if not hasattr(TL.LightningModuleBase, "device"):
            device = torch.device("cpu")

        @property
        def current_epoch(self):
            return self.trainer.current_epoch

        def configure_optimizers(self):
            return torch.optim.SGD([self.w], lr=0.1)

        def training_step(self, batch, batch_idx):
            return {"loss": 0.0}

    return Toy()


def test_schedule_through_minitrainer_against_the_reference(state_dir):
    """For every recorded val_every_n_* / skip_first_n_epochs setting: the batches and epochs that evaluate, and val_accuracy /
    val_episode_return of every epoch (-inf where none ran), with 6 epochs of 4 batches driven by MiniTrainer.fit."""
    from tacorl_amd import lightning as TL

    for case in _golden()["schedule"]:
        cb = _callback(state_dir, "episodes", **case["settings"])
        rows = []

        class Probe:
            def on_train_batch_end(self, trainer, pl_module, outputs, batch, batch_idx):
                rows.append(["batch", trainer.current_epoch, batch_idx, self.n != len(getattr(cb, "asked", []))])
                self.n = len(getattr(cb, "asked", []))

            def on_train_batch_start(self, trainer, pl_module, batch, batch_idx):
                self.n = len(getattr(cb, "asked", []))

            def on_train_epoch_end(self, trainer, pl_module):
                lm = trainer.logged_metrics
                rows.append(["epoch", trainer.current_epoch, -1, self.n != len(getattr(cb, "asked", [])), lm["val_accuracy"],
                             lm["val_episode_return"]])

        tr = TL.MiniTrainer(max_epochs=6, callbacks=[cb, Probe()])
        tr.fit(_toy(_Env()), [torch.zeros(1)] * 4)
        want = [[_unwrap(v) for v in r] for r in case["rows"]]
        assert len(rows) == len(want) == 6 * 5
        for got, w in zip(rows, want):
            assert got[:4] == w[:4], (case["settings"], got, w)
            if got[0] == "epoch":
                assert got[4] == pytest.approx(w[4], rel=1e-12) and got[5] == pytest.approx(w[5], rel=1e-12), (case["settings"], got, w)
        if "val_every_n_batches" in case["settings"]:
            assert any(k.startswith("batch_val/") for k in tr.logged_metrics)


def test_d4rl_callback_publishes_the_score_and_minus_infinity(state_dir):
    from tacorl_amd import lightning as TL
    from tacorl_amd.utils.callbacks.rollout_d4rl import Rollout

    cb = _scripted(Rollout)(rollout_manager={"_target_": "tacorl.evaluation.rollout_manager_d4rl.LatentPlanRollout"},
                            val_episodes=4, val_every_n_epochs=2, envs=[_Env()])
    seen = []

    class Probe:
        def on_train_epoch_end(self, trainer, pl_module):
            seen.append({k: trainer.logged_metrics[k] for k in ("val_accuracy", "val_episode_return", "val_score")})

    tr = TL.MiniTrainer(max_epochs=2, callbacks=[cb, Probe()])
    tr.fit(_toy(), [torch.zeros(1)] * 2)
    infos = [E.scripted_info("episode", k) for k in range(4)]
    ret = float(np.mean([i["episode_return"] for i in infos]))
    assert seen[0] == {"val_accuracy": sum(i["success"] for i in infos) / 4, "val_episode_return": ret, "val_score": 2.0 * ret}
    assert seen[1] == {k: float("-inf") for k in seen[1]}
    assert tr.logged_metrics["validation/score"] == 2.0 * ret


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(state_dir):
    from tacorl_amd.utils.callbacks import rollout as M
    from tacorl_amd.utils.callbacks.rollout_d4rl import Rollout as RolloutD4RL

    with pytest.raises(AssertionError, match="val_every_n ... is not set") as e:
        M.Rollout(rollout_manager=MANAGER, eval_strategy="episodes")
    assert str(e.value) == _golden()["no_schedule_message"]
    with pytest.raises(ValueError, match="RLRollout, LatentPlanRollout, TACORL, RelayImitationLearning"):
        M.Rollout(rollout_manager={"_target_": "tacorl.evaluation.rollout_manager.RolloutLongHorizon"}, val_every_n_epochs=1,
                  eval_strategy="episodes")
    with pytest.raises(ValueError, match="rollout_manager_d4rl"):
        RolloutD4RL(rollout_manager=MANAGER, val_every_n_epochs=1)
    cb = M.Rollout(rollout_manager=MANAGER, val_every_n_epochs=1, eval_strategy="episodes")
    with pytest.raises(ValueError, match=r"envs=\[env0, env1, \.\.\.\]"):
        cb.on_fit_start(None, _Module(env=None))
    cb.on_fit_start(None, _Module(env=_Env()))  # pl_module.env alone
    assert len(cb.envs) == 1
    with pytest.raises(ValueError, match="n_envs"):
        M.Rollout(rollout_manager=MANAGER, val_every_n_epochs=1, eval_strategy="episodes", envs=lambda i: _Env())
    assert len(M.Rollout(rollout_manager=MANAGER, val_every_n_epochs=1, eval_strategy="episodes", envs=lambda i: _Env(), n_envs=3).envs) == 3
    # an empty group: the reference divides by zero (:219-221)
    info = dict(episode_length=3, episode_return=-1.0, success=True)
    with pytest.raises(ValueError, match="dynamic group"):
        M.grouped_metrics([("open_drawer", [info])])
    with pytest.raises(ValueError, match="static group"):
        M.grouped_metrics([("move_block_left", [info])])
    with pytest.raises((AssertionError, FileNotFoundError)):
        M.Rollout(rollout_manager=MANAGER, val_every_n_epochs=1, data_dir=os.path.join(state_dir, "missing"))


def test_ingest_refuses_what_the_augment_reader_refuses():
    """FrameIngest reads the validation list with data/augment.py's reader: same refusal, same message."""
    from tacorl_amd.data.augment import augment_specs
    from tacorl_amd.evaluation import frame_ingest as F

    class Surf:
        cams, goal_cams, net = ["rgb_static"], ["rgb_static"], object()

    class Mod:
        dev, compute, img_dtype = "cpu", 0, torch.float32
        plan_proposal_obs_modalities = plan_proposal_goal_modalities = action_decoder_modalities = ["rgb_static"]

    m = Mod()
    m.__dict__["_actor_surface"] = Surf()
    for bad in ([{"_target_": "torchvision.transforms.CenterCrop", "size": 64}],
                [{"_target_": "torchvision.transforms.Normalize", "mean": [0.4], "std": [0.5]}]):
        cfg = {"transforms": {"validation": {"rgb_static": bad}}}
        with pytest.raises(NotImplementedError) as want:
            augment_specs(cfg, ["rgb_static"], "validation")
        with pytest.raises(NotImplementedError) as got:
            F.FrameIngest(m, 2, cfg)
        assert str(got.value) == str(want.value)
    with pytest.raises(NotImplementedError, match="draws an augmentation"):
        F.FrameIngest(m, 2, {"transforms": {"validation": {"rgb_static": [{"_target_": "tacorl.utils.transforms.RandomShiftsAug", "pad": 4}]}}})
    with pytest.raises(ValueError, match="no image rollout surface"):
        F.FrameIngest(object(), 2, None)


# ------------------------------------------------------------------------------------------ keyed draws
def test_keyed_draws_depend_on_their_key_alone():
    from tacorl_amd.utils.callbacks.rollout import keyed_generator

    a = torch.randn(4, generator=keyed_generator(3, (1, 2), "plan", 0))
    torch.manual_seed(99)
    torch.rand(7)
    assert torch.equal(a, torch.randn(4, generator=keyed_generator(3, (1, 2), "plan", 0)))
    for other in ((4, (1, 2), "plan", 0), (3, (1, 3), "plan", 0), (3, (1, 2), "cem", 0), (3, (1, 2), "plan", 1)):
        assert not torch.equal(a, torch.randn(4, generator=keyed_generator(*other)))
