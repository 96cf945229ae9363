"""The long-horizon rollout evaluation on the GPU.

  * tacorl_noise_fill_rows (csrc/noise_ops.hip) against tacorl_amd.noise.philox_rows_restatement: uniforms bit for bit, normals
    inside tests/noise_ref.py's bound (the one tacorl_noise_fill is held to), for 1, 3 and 64 rows of arbitrary episodes at
    their own steps and ragged / whole / multi-group rows; masked rows untouched bit for bit; a row's bits independent of the
    batch around it; every refusal with nothing written;
  * rollout_episodes_refill on real policies: an episode's actions are the same bits alone, in a refilled queue over two slots
    and in fixed batches of two - the D4RL latent-plan module with a sampled plan, TACORL with CEM, the image module through
    FrameIngest;
  * RolloutLongHorizon.run_and_log_validation end to end."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tacorl_amd import noise as N
from tests import d4rl_cfg as K
from tests import noise_ref as NR
from tests import rollout_envs as E
from tests import rollout_lh_envs as LH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x0123_4567_89AB_CDEF
SENTINEL = 0x7FC0DEAD  # a NaN with a payload: an untouched float holds exactly these bits
EINVAL = -22
INNERS = [1, 3, 4, 5, 16, 70]


def _sentinel(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _bits(t):
    return t.view(torch.int32).cpu().numpy()


def _rows(R, seed=1):
    """Arbitrary episodes (not consecutive, with repeats where R allows), per-row steps and plan numbers that differ."""
    g = np.random.RandomState(seed)
    ep = g.randint(0, 1 << 31, size=R).astype(np.int64) * 2 + g.randint(0, 2, size=R)
    if R >= 3:
        ep[R - 1] = ep[0]  # a repeated episode, at another step
    return ep.tolist(), g.randint(0, 300, size=R).tolist(), g.randint(0, 75, size=R).tolist()


def _carve(R, specs, pad=4):
    """specs: (kind, draw, inner, which, rows) -> (segments, n_f32); every buffer on a multiple of 4 floats, `pad` behind it."""
    segs, off = [], 0
    for kind, draw, inner, which, rows in specs:
        segs.append(N.RowSegment(off, kind, draw, inner, which, rows))
        off = NR.al4(off + R * inner) + pad
    return segs, off


def _check(buf, R, rows, segs):
    """Every segment of a filled buffer against the restatement; returns (written mask, worst normal error / bound)."""
    ep, steps, plan_nos = rows
    f32 = buf.cpu().numpy()
    written, worst = np.zeros(f32.size, bool), 0.0
    for s in segs:
        drawn = list(range(R)) if s.rows is None else sorted(set(s.rows))
        want = N.philox_rows_restatement(SEED, s.draw_id, s.kind, ep, plan_nos if s.which == N.BY_PLAN else steps, s.inner)[:, 0]
        got = f32[s.offset: s.offset + R * s.inner].reshape(R, s.inner)
        for r in drawn:
            written[s.offset + r * s.inner: s.offset + (r + 1) * s.inner] = True
            if s.kind == N.NORMAL:
                assert np.isfinite(got[r]).all()
                worst = max(worst, float((np.abs(got[r].astype(np.float64) - want[r]) / NR.normal_bound(want[r])).max()))
            else:
                assert (got[r].astype(np.float64) == want[r]).all() and (got[r] == want[r].astype(np.float32)).all(), (s.draw_id, r)
    assert worst <= 1.0, worst
    assert (_bits(buf)[~written] == np.int32(SENTINEL)).all()
    return written, worst


# ------------------------------------------------------------------------------------------ kernel vs restatement
@pytest.mark.parametrize("R", [1, 3, 64])
def test_rows_kernel_against_the_restatement(R):
    rows = _rows(R)
    worst = 0.0
    for inner in INNERS:
        segs, n = _carve(R, [("uniform", "ro_rand_a", inner, N.BY_STEP, None), ("normal", "ro_plan", inner, N.BY_PLAN, None)])
        buf = _sentinel(n)
        N.RowNoise(SEED).fill(rows, segs, buf)
        torch.cuda.synchronize()
        written, w = _check(buf, R, rows, segs)
        assert written.sum() == 2 * R * inner and (~written).sum() >= 8
        worst = max(worst, w)
    print(f"R {R}: worst |z_gpu - z_fp64| / bound = {worst:.4f} (K = {NR.K})")


@pytest.mark.parametrize("R", [3, 64])
def test_a_step_s_four_segments_in_one_launch(R):
    """Da K = 70 and Da = 7 uniforms for every row, P = 16 and iters N P = 2 * 3 * 5 = 30 normals for the rows that re-plan."""
    rows = _rows(R, seed=2)
    due = [1] if R == 3 else [0, 5, 31, 32, 63]
    segs, n = _carve(R, [("uniform", "ro_rand_a", 70, N.BY_STEP, None), ("uniform", "ro_rand_b", 7, N.BY_STEP, None),
                         ("normal", "ro_plan", 16, N.BY_PLAN, due), ("normal", "ro_cem", 30, N.BY_PLAN, due)])
    buf = _sentinel(n)
    N.RowNoise(SEED).fill(rows, segs, buf)
    torch.cuda.synchronize()
    written, _ = _check(buf, R, rows, segs)
    assert written.sum() == R * 77 + len(due) * 46
    # the two draws of a kind are different streams, and the two numbers are used where they are asked for
    f32 = buf.cpu().numpy()
    assert not np.array_equal(f32[segs[0].offset: segs[0].offset + 7], f32[segs[1].offset: segs[1].offset + 7])


def test_masks_leave_the_other_rows_alone():
    R, rows = 5, _rows(5, seed=3)
    specs = lambda m: [("uniform", "ro_rand_a", 6, N.BY_STEP, m[0]), ("normal", "ro_cem", 9, N.BY_PLAN, m[1]),  # noqa: E731
                       ("normal", "ro_plan", 4, N.BY_PLAN, m[2])]
    for masks in (([0, 4], [2], []), ([], [], [3]), ([1, 2, 3], [0, 1, 2, 3, 4], [0])):  # (empty segments in every position)
        segs, n = _carve(R, specs(masks))
        buf = _sentinel(n)
        N.RowNoise(SEED).fill(rows, segs, buf)
        torch.cuda.synchronize()
        written, _ = _check(buf, R, rows, segs)  # (checks that everything outside the masks holds the sentinel's bits)
        assert written.sum() == 6 * len(masks[0]) + 9 * len(masks[1]) + 4 * len(masks[2])
    segs, n = _carve(R, specs(([], [], [])))
    buf = _sentinel(n)
    N.RowNoise(SEED).fill(rows, segs, buf)
    torch.cuda.synchronize()
    assert (_bits(buf) == np.int32(SENTINEL)).all()


def test_a_row_s_bits_do_not_depend_on_the_batch():
    ep, step, plan_no = 123456789, 17, 4
    specs = [("uniform", "ro_rand_a", 70, N.BY_STEP, None), ("normal", "ro_plan", 16, N.BY_PLAN, None),
             ("normal", "ro_cem", 30, N.BY_PLAN, None)]
    got = {}
    for R, r in ((1, 0), (3, 0), (64, 63)):
        rows = _rows(R, seed=4)
        rows[0][r], rows[1][r], rows[2][r] = ep, step, plan_no
        segs, n = _carve(R, specs)
        buf = _sentinel(n)
        N.RowNoise(SEED).fill(rows, segs, buf)
        torch.cuda.synchronize()
        b = _bits(buf)
        got[R] = [b[s.offset + r * s.inner: s.offset + (r + 1) * s.inner].tobytes() for s in segs]
    assert got[1] == got[3] == got[64]
    assert len(set(got[1][1:])) == 2


def test_refusals_write_nothing():
    from tacorl_amd import _lib

    L = _lib.lib()
    R, n = 3, 64
    buf = _sentinel(n + 4)
    rows = _rows(R)
    seg = lambda **kw: N.RowSegment(**{**dict(offset=0, kind="normal", draw_id=98, inner=7), **kw})  # noqa: E731

    def table(segs=None, **fields):
        t = N.rows_table(rows, [seg()] if segs is None else segs, n)
        for k, v in fields.items():
            setattr(t, k, v)
        return t

    def seg_field(**fields):
        t = table()
        for k, v in fields.items():
            setattr(t.seg[0], k, v)
        return t

    base = C.c_void_p(buf.data_ptr())
    bad = {"no rows": table(n_rows=0), "65 rows": table(n_rows=65), "five segments": table(n_seg=5), "no segment": table(n_seg=0),
           "draw id 65536": seg_field(draw_id=65536), "draw id -1": seg_field(draw_id=-1), "inner 0": seg_field(inner=0),
           "past n_f32": table([seg(), seg(offset=44)]),          # 3 * 7 floats from 44: one past the buffer's 64
           "offset -4": seg_field(offset=-4), "mask bit 3 of 3 rows": seg_field(mask=0b1001), "mask bit 63 of 3 rows": seg_field(mask=1 << 63),
           "kind keep": seg_field(kind=N.KEEP), "which 2": seg_field(which=2)}
    for name, t in bad.items():
        assert L.tacorl_noise_fill_rows(C.byref(t), base, 1, _lib.stream()) == EINVAL, name
    ok = table()
    assert L.tacorl_noise_fill_rows(C.byref(ok), C.c_void_p(buf.data_ptr() + 4), 1, _lib.stream()) == EINVAL  # 4-byte aligned base
    assert L.tacorl_noise_fill_rows(C.byref(ok), None, 1, _lib.stream()) == EINVAL
    with pytest.raises(_lib.TacorlHipError):
        N.RowNoise(1).fill(rows, [seg(offset=44)], buf[:n])
    torch.cuda.synchronize()
    assert (_bits(buf) == np.int32(SENTINEL)).all()
    # ... and the table that ends exactly at n_f32 is taken, as is a mask of all 64 rows
    N.RowNoise(1).fill(rows, [seg(), seg(offset=43)], buf[:n])
    full = _sentinel(64 * 4)
    N.RowNoise(1).fill(_rows(64), [seg(inner=4)], full)
    torch.cuda.synchronize()
    b = _bits(buf)
    assert (b[21:43] == np.int32(SENTINEL)).all() and (b[n:] == np.int32(SENTINEL)).all()
    assert torch.isfinite(buf[:21]).all() and torch.isfinite(buf[43:n]).all() and torch.isfinite(full).all()


# ------------------------------------------------------------------------------------------ refill on real policies
LENGTHS = [3, 9, 4, 17, 6]


def _queue(policy_of, envs_of, episodes, seed=11):
    """The three runs: every episode alone (a queue over ONE slot), refilled over two slots, fixed batches of two."""
    from tacorl_amd.evaluation.vec_policy import rollout_episodes_refill
    from tacorl_amd.utils.callbacks.rollout_long_horizon import row_noise

    runs = {}
    with torch.no_grad():
        for name, R, refill in (("alone", 1, True), ("refill", 2, True), ("batches", 2, False)):
            pol, ingest = policy_of(R)
            acts = []
            infos = rollout_episodes_refill(pol, envs_of(R), episodes, noise=row_noise(pol, seed), ingest=ingest, actions_out=acts,
                                            refill=refill)
            runs[name] = (infos, acts)
    return runs


def _same_episodes(runs, lengths=None):
    infos, acts = runs["alone"]
    if lengths is not None:
        assert [i["episode_length"] for i in infos] == lengths
    for other in ("refill", "batches"):
        oi, oa = runs[other]
        assert [(i["episode_length"], i["episode_return"], i["success"], i.get("successful_tasks")) for i in oi] == \
               [(i["episode_length"], i["episode_return"], i["success"], i.get("successful_tasks")) for i in infos], other
        for e, (x, y) in enumerate(zip(acts, oa)):
            assert len(x) == len(y) and all(p.tobytes() == q.tobytes() for p, q in zip(x, y)), (other, e)
    # episodes differ from one another (other starts, other draws), so the comparison above is not between constants
    assert not np.array_equal(acts[0][0], acts[1][0])


def _d4rl(kind):
    torch.manual_seed(5)
    lmp = K.build(K.playlmp_d4rl_cfg(latent=16, T=8, device=DEV, dropout_p=0.0))
    mod = lmp if kind == "playlmp_d4rl" else K.build(K.tacorl_d4rl_cfg(play_lmp=lmp, device=DEV))
    mod.eval()
    return mod


@pytest.mark.parametrize("use_cem", [False, True], ids=["sampled_plan", "tacorl_cem"])
def test_refilling_changes_no_episode_of_a_latent_plan_policy(use_cem):
    from tacorl_amd.evaluation.vec_policy import LatentPlanPolicy

    mod = _d4rl("tacorl_d4rl" if use_cem else "playlmp_d4rl")
    assert 2 <= mod.ad.ROWS_KERNEL_MAX_R  # every run below is on the rows kernel, whose rows are batch-independent
    kw = dict(use_cem=True, cem_kwargs=dict(batch_size=64, num_iterations=2)) if use_cem else {}  # 64: the smallest population
    episodes = [(40 + 3 * i, {"length": n, "seed": i, "tasks": [LH.A, LH.B]}) for i, n in enumerate(LENGTHS)]
    runs = _queue(lambda R: (LatentPlanPolicy(mod, R, plan_duration=4, **kw), None),
                  lambda R: [LH.ScriptedVectorEnv() for _ in range(R)], episodes)
    _same_episodes(runs, LENGTHS)
    # another seed, other episodes: the draws reach the actions
    other = _queue(lambda R: (LatentPlanPolicy(mod, R, plan_duration=4, **kw), None),
                   lambda R: [LH.ScriptedVectorEnv() for _ in range(R)], episodes[:1], seed=12)
    assert not np.array_equal(other["alone"][1][0][0], runs["alone"][1][0][0])


def test_refilling_through_the_frame_ingest():
    """Three episodes over two slots on the image module: the refilled row's goal is encoded anew, its neighbour's kept."""
    from tacorl_amd.evaluation.frame_ingest import FrameIngest
    from tacorl_amd.evaluation.vec_policy import LatentPlanPolicy
    from tests.test_rollout_callback_gpu import DUR, MAX_STEPS, SRC, _tm, build

    class Env(E.GridImageEnv):
        """The episode's step limit comes with its reset, so an episode is the same in any slot."""

        def reset(self, task_info=None, limit=MAX_STEPS):
            self._max_episode_steps = int(limit)
            return super().reset(task_info)

    mod = build("playlmp")
    mod.eval()
    info = lambda s, e, n: {"task_info": {"start_info": E.state_of_step(s), "goal_info": E.state_of_step(e), "tasks": [LH.A]},  # noqa: E731
                            "limit": n}
    # slot 0 takes the third episode at step 3, while slot 1 is in the middle of the second
    episodes = [(7, info(100, 120, 3)), (8, info(200, 263, MAX_STEPS)), (9, info(300, 317, 5))]
    runs = _queue(lambda R: (LatentPlanPolicy(mod, R, plan_duration=DUR), FrameIngest(mod, R, _tm())),
                  lambda R: [Env(seed=0, src_hw=SRC, threshold=1) for _ in range(R)], episodes)
    _same_episodes(runs)
    lengths = [i["episode_length"] for i in runs["alone"][0]]
    assert all(1 <= n <= m for n, m in zip(lengths, (3, MAX_STEPS, 5))) and lengths[1] > lengths[0]


# ------------------------------------------------------------------------------------------ end to end
def test_long_horizon_callback_end_to_end(tmp_path):
    from tacorl_amd.utils.callbacks.rollout_long_horizon import RolloutLongHorizon

    root = str(tmp_path)
    E.write_state_dir(root, LH.START_END_TASKS)
    with open(os.path.join(root, "tasks.json"), "w") as f:
        json.dump(LH.START_END_TASKS, f)
    mod = _d4rl("playlmp_d4rl")

    class Sink:
        def __init__(self):
            self.logged = {}

        def __getattr__(self, name):
            return getattr(mod, name)

        def log(self, name, value, **kw):
            self.logged[name] = float(value)

    class _Trainer:
        datamodule = None

    def run(R, refill):
        cb = RolloutLongHorizon(num_rollouts=LH.NUM_ROLLOUTS, tasks_per_rollout=2, refill=refill, val_every_n_epochs=1,
                                rollout_manager={"_target_": "tacorl.evaluation.rollout_manager_d4rl.LatentPlanRollout", "plan_duration": 4},
                                data_dir=root, start_end_tasks=os.path.join(root, "tasks.json"), max_episode_steps=12, seed=3,
                                envs=[LH.ScriptedVectorEnv() for _ in range(R)])
        sink = Sink()
        cb.on_fit_start(_Trainer(), mod)
        val_info = cb.run_and_log_validation(sink, on_step=False, on_epoch=True)
        return cb, sink.logged, val_info

    cb, logged, val_info = run(3, True)
    infos = cb.last_infos
    assert len(infos) == len(cb.last_actions) == LH.NUM_ROLLOUTS and all(e._max_episode_steps == 12 for e in cb.envs)
    windows = [cb.rollout_tasks[g % len(cb.rollout_tasks)] for g in range(LH.NUM_ROLLOUTS)]
    assert [i["episode_length"] for i in infos] == [min(12, 3 + w["seq_len"] % 11) for w in windows]
    # the reference's aggregation (rollout_long_horizon.py:69, :106-117) on the same infos
    per = np.array([0] * 2)
    for i in infos:
        if len(i["successful_tasks"]) > 0:
            per[: len(i["successful_tasks"])] += 1
    want = {"validation/LH_avg_episode_return": np.mean([i["episode_return"] for i in infos]),
            "validation/LH_avg_episode_length": np.mean([i["episode_length"] for i in infos]),
            "validation/LH_1_accuracy": per[0] / len(infos), "validation/LH_2_accuracy": per[1] / len(infos)}
    assert set(logged) == set(want) and all(logged[k] == float(v) for k, v in want.items()), (logged, want)
    assert 1.0 >= logged["validation/LH_1_accuracy"] >= logged["validation/LH_2_accuracy"] >= 0.0
    assert val_info == {k.split("/", 1)[1]: v for k, v in logged.items()} and mod.training
    # fixed batches and another number of slots: the same episodes, the same numbers
    for R, refill in ((3, False), (2, True)):
        cb2, logged2, _ = run(R, refill)
        assert logged2 == logged, (R, refill)
        for x, y in zip(cb.last_actions, cb2.last_actions):
            assert len(x) == len(y) and all(p.tobytes() == q.tobytes() for p, q in zip(x, y)), (R, refill)
