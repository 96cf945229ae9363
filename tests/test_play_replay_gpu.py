"""The resident play replay on the GPU: the sampler kernel (`tacorl_sample_play_windows`) against the host PlayIndex.sample +
pad_actions and the reference's recorded items bit for bit, HbmPlayReplay's two batch forms against HbmReplay's, TACORL /
PlayLMP steps fed by them - the fused batch, the gathered batch and the parent's HbmReplay batch must be one step - and
Trainer.fit(datamodule=PlayDataModule) through the pytorch_lightning stand-in."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests.proc_util import run_group

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "play_sampler.npz"))
CFG = json.loads(str(G["cfg"]))
EP, N = [[0, 99], [100, 189], [190, 299]], 310  # the synthetic dataset: three episodes, ten frames behind the last one
U_TOP = 1.0 - 2.0 ** -53                        # the largest double below 1


def _actions(A, n=N, seed=4):
    a = np.random.RandomState(seed + A).uniform(-1, 1, size=(n, A)).astype(np.float32)
    a[:, -1] = np.where(a[:, -1] >= 0, 1.0, -1.0)
    return a


def _nn(kind):
    """full: every frame has 1..5 neighbours; partial: the lists of frames < 150 only, half of them empty; none."""
    rs = np.random.RandomState(8)
    if kind == "full":
        return {k: rs.randint(0, 300, size=rs.randint(1, 6)).tolist() for k in range(300)}
    if kind == "partial":
        return {k: rs.randint(0, 300, size=rs.randint(1, 6) if k % 2 else 0).tolist() for k in range(150)}
    return None


def _index(min_ws, max_ws, goal_aug=False, nn="full", ep=EP):
    from tacorl_amd.data.replay import PlayIndex

    return PlayIndex(ep, min_ws, max_ws, goal_sampling_prob=0.3, goal_augmentation=goal_aug, nn_steps_from_step=_nn(nn))


def _run(ix, acts, draws, **kw):
    """(replay, ids (B, T), goal (B), actions, disp, window_size as numpy) of one sampler launch, nothing but tables resident."""
    from tacorl_amd.data.play_replay import HbmPlayReplay

    rp = HbmPlayReplay({}, acts, ix, device=DEV, batch_size=4, **kw)
    b = rp.batch(draws, fused=True)
    torch.cuda.synchronize()
    B, T = b["replay"]["B"], b["replay"]["T"]
    ids = b["replay"]["ids"].cpu().numpy()
    assert ids.shape == (B * T + B,) and T == ix.max_ws and b["actions"].shape == (B, T, acts.shape[1])
    return rp, {"frames": ids[: B * T].reshape(B, T), "goal": ids[B * T:], "actions": b["actions"].cpu().numpy(),
                "disp": b["disp"].cpu().numpy(), "window_size": b["window_size"].cpu().numpy()}


def _assert_equals_host(ix, acts, draws, status=0):
    from tacorl_amd.data.replay import pad_actions

    host = {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in draws.items()}
    s = ix.sample(host["idx"], host)
    rp, got = _run(ix, acts, draws)
    for k in ("frames", "goal", "disp", "window_size"):
        assert np.array_equal(got[k], s[k]), (k, got[k], s[k])
    assert np.array_equal(got["actions"], pad_actions(acts, s["frames"], s["padded"]))
    assert got["frames"].min() >= 0 and max(got["frames"].max(), got["goal"].max()) < rp.tables["n_frames"] and got["goal"].min() >= 0
    assert int(rp.status.item()) == status
    return got, s


def _fresh_draws(ix, n, seed):
    """ix.draw + idx, the first items carrying the extremes: the first / last item, the uniforms 0.0 and 1 - 2^-53."""
    rng = np.random.default_rng(seed)
    d = ix.draw(n, rng)
    d["idx"] = rng.integers(0, len(ix), size=n)
    d["idx"][: min(n, 2)] = [0, len(ix) - 1][: min(n, 2)]
    for k in ("u_choice", "u_random_state"):
        d[k][: min(n, 2)] = [0.0, U_TOP][: min(n, 2)]
    return d


# ------------------------------------------------------------------------------------------------------------ the kernel
def _named(rec, goal_aug):
    """tests/test_sampler_cpu.py::_draws: name the reference's recorded numpy draws of one item."""
    it = iter(rec)
    d = {"window_size": int(next(it)[1])}
    u = next(it)[1]
    d["strategy"] = 0 if u < CFG["strategy"]["geometric"] else 1
    d.update(disp=1, noise_step=0, u_choice=0.0, u_random_state=0.0)
    if d["strategy"] == 0:
        d["disp"] = int(next(it)[1])
        if goal_aug:
            d["noise_step"] = int(next(it)[1]) - 1
    else:
        _, u2 = next(it)
        d["u_choice"] = d["u_random_state"] = u2
    assert next(it, None) is None
    return d


@pytest.mark.parametrize("variant,goal_aug", [("plain", False), ("goal_aug", True)])
def test_kernel_equals_the_reference_dataset_on_the_recorded_draws(variant, goal_aug):
    from tacorl_amd.data.replay import PlayIndex

    ix = PlayIndex(G["ep"], CFG["min_ws"], CFG["max_ws"], goal_sampling_prob=CFG["p"], goal_strategy_prob=CFG["strategy"],
                   goal_augmentation=goal_aug, nn_steps_from_step=json.loads(str(G["nn"])))
    ds = [_named(r, goal_aug) for r in json.loads(str(G[f"{variant}/draws"]))]
    draws = {k: np.array([d[k] for d in ds]) for k in ds[0]}
    draws["idx"] = np.asarray(G[f"{variant}/idx"], dtype=np.int64)
    rp, got = _run(ix, np.asarray(G["all_actions"], np.float32), draws)
    assert np.array_equal(got["window_size"], G[f"{variant}/window_size"])
    assert np.array_equal(got["frames"], G[f"{variant}/frames"])
    assert np.array_equal(got["goal"], G[f"{variant}/goal"])
    assert np.array_equal(got["disp"], G[f"{variant}/disp"])
    assert np.array_equal(got["actions"], G[f"{variant}/actions"])
    assert int(rp.status.item()) == 0
    rp.check()


@pytest.mark.parametrize("min_ws,max_ws", [(1, 1), (8, 16), (16, 16), (2, 64)])
def test_kernel_equals_host_sampler_on_fresh_draws(min_ws, max_ws):
    """One wavefront per window, four windows per block: B = 1, 3, 4, 5 (a block less one, a full block, a block and one)
    and 257; a window of one frame, the yaml's 8..16, the constant 16 and 2..64 (a full wavefront of frames); two action
    widths; with and without goal augmentation; a full neighbour table, one with empty lists and missing keys, none."""
    for n in (1, 3, 4, 5, 257):
        for A in (7, 3):
            acts = _actions(A)
            for goal_aug in (False, True):
                for nn in ("full", "partial", "none"):
                    ix = _index(min_ws, max_ws, goal_aug, nn)
                    got, s = _assert_equals_host(ix, acts, _fresh_draws(ix, n, 100 * n + A))
                    if n == 257 and min_ws < max_ws:
                        assert s["padded"].any() and (~s["padded"][:, -1]).any() and (s["disp"] == -1).any() and (s["disp"] > 0).any()


def _one(ix, **over):
    """Four copies of one draw by construction (a full block)."""
    d = dict(idx=0, window_size=ix.max_ws, strategy=0, disp=1, noise_step=0, u_choice=0.0, u_random_state=0.0)
    d.update(over)
    return {k: np.full(4, v, dtype=np.float64 if k.startswith("u_") else np.int64) for k, v in d.items()}


def test_edge_cases_by_construction():
    acts = _actions(7)
    # a one-frame window at frame 0 with noise_step = -1: the goal clips to 0 and the status stays 0
    ix = _index(1, 4, goal_aug=True)
    got, _ = _assert_equals_host(ix, acts, _one(ix, idx=0, window_size=1, noise_step=-1))
    assert (got["goal"] == 0).all() and (got["frames"] == 0).all() and (got["window_size"] == 1).all()
    for nz in (0, 1):
        got, _ = _assert_equals_host(ix, acts, _one(ix, idx=0, window_size=1, noise_step=nz, disp=2 ** 62))
        assert (got["goal"] == nz).all()  # stride 0: the displacement does not count, and nothing is divided by it
    # disp = 2^62: the goal is the episode end (window 2: the host's own product start + disp does not overflow either)
    ix = _index(2, 16, goal_aug=True)
    for nz in (-1, 0, 1):
        got, _ = _assert_equals_host(ix, acts, _one(ix, idx=len(ix) - 1, window_size=2, disp=2 ** 62, noise_step=nz))
        assert (got["goal"] == 299).all() and (got["disp"] == 2 ** 62).all()
        # a longer window: (ws - 1) * disp wraps in int64 on the host (PlayIndex.sample is not defined there); the kernel
        # decides `far` before it multiplies and answers min(end, .) = the end
        rp, got = _run(ix, acts, _one(ix, idx=5, window_size=16, disp=2 ** 62, noise_step=nz))
        assert (got["goal"] == 99).all() and int(rp.status.item()) == 0
    # the last step inside the episode, with and without the noise step pushing it over the end
    for nz, want in ((-1, 98), (0, 99), (1, 99)):
        got, _ = _assert_equals_host(ix, acts, _one(ix, idx=0, window_size=10, disp=11, noise_step=nz))
        assert (got["goal"] == want).all()
    # similar_robot_obs: a key beyond the table and an empty list take the random state, whatever u_choice says
    ix = _index(8, 16, nn="partial")
    look = ix.episode_lookup
    beyond, empty, filled = int(np.flatnonzero(look == 150)[0]), int(np.flatnonzero(look == 3)[0]), int(np.flatnonzero(look == 4)[0])
    for idx, ws in ((beyond, 8), (empty, 8)):  # keys 157 (outside the table of 150 keys) and 10 (an empty list)
        got, _ = _assert_equals_host(ix, acts, _one(ix, idx=idx, window_size=ws, strategy=1, u_choice=0.7, u_random_state=0.5))
        assert (got["goal"] == look[len(look) // 2]).all() and (got["disp"] == -1).all()
        got, _ = _assert_equals_host(ix, acts, _one(ix, idx=idx, window_size=ws, strategy=1, u_random_state=U_TOP))
        assert (got["goal"] == look[-1]).all()
    # u = 1 - 2^-53: the last element of the list, never one past it (key 11)
    got, _ = _assert_equals_host(ix, acts, _one(ix, idx=filled, window_size=8, strategy=1, u_choice=U_TOP))
    assert (got["goal"] == _nn("partial")[11][-1]).all()
    got, _ = _assert_equals_host(ix, acts, _one(ix, idx=filled, window_size=8, strategy=1, u_choice=0.0))
    assert (got["goal"] == _nn("partial")[11][0]).all()
    # a neighbour behind the last episode end (frames 300..309 exist) is clipped to it by the definition: no status
    from tacorl_amd.data.replay import PlayIndex

    ix = PlayIndex(EP, 8, 16, nn_steps_from_step={7: [305]})
    got, _ = _assert_equals_host(ix, acts, _one(ix, idx=0, window_size=8, strategy=1))
    assert (got["goal"] == 299).all()


def test_draws_outside_the_index_are_clamped_and_reported():
    acts = _actions(7)
    ix = _index(8, 16, goal_aug=True)
    d = _fresh_draws(ix, 6, 9)
    _assert_equals_host(ix, acts, d, status=0)  # in-range draws leave the status word 0
    for key, vals, clamped in (("idx", [-1, len(ix)], [0, len(ix) - 1]), ("window_size", [0, 17], [8, 16]),
                               ("strategy", [7, -2], [1, 0]), ("disp", [0, -5], [1, 1]), ("noise_step", [-4, 9], [-1, 1])):
        bad, ok = dict(d), dict(d)
        bad[key], ok[key] = d[key].copy(), d[key].copy()
        bad[key][:2], ok[key][:2] = vals, clamped
        if key in ("disp", "noise_step"):
            bad["strategy"] = ok["strategy"] = np.zeros(6, np.int64)  # (read for a geometric goal only)
        s = ix.sample(ok["idx"], ok)
        rp, got = _run(ix, acts, bad)
        assert int(rp.status.item()) == 1, key
        with pytest.raises(IndexError):
            rp.check()
        assert np.array_equal(got["frames"], s["frames"]) and np.array_equal(got["goal"], s["goal"]), key
        assert np.array_equal(got["window_size"], s["window_size"]) and np.array_equal(got["disp"], s["disp"]), key
        assert got["frames"].min() >= 0 and got["frames"].max() < N and got["goal"].min() >= 0 and got["goal"].max() < N
        rp.batch(d)  # the status word is never cleared by a clean batch
        assert int(rp.status.item()) == 1


def test_entry_point_refuses_bad_arguments_without_launching():
    from tacorl_amd import _lib
    from tacorl_amd.data.play_replay import HbmPlayReplay

    ix = _index(8, 16, goal_aug=True)
    rp = HbmPlayReplay({}, _actions(7), ix, device=DEV, batch_size=8)
    t, n, T = rp.tables, 8, 16
    d = ix.draw_device(n, DEV, torch.Generator(device=DEV).manual_seed(0))
    ids = torch.full((n * T + n,), -7, dtype=torch.int64, device=DEV)
    act = torch.full((n, T, 7), -7.0, device=DEV)
    dsp, ws = torch.full((n,), -7, dtype=torch.int64, device=DEV), torch.full((n,), -7, dtype=torch.int64, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    off = lambda x, k: C.c_void_p(x.data_ptr() + k)  # noqa: E731

    def args(**over):
        a = dict(lookup=p(t["lookup"]), n_items=t["lookup"].numel(), es=p(t["ep_start"]), ee=p(t["ep_end"]), n_ep=t["ep_start"].numel(),
                 nn_ptr=p(t["nn_ptr"]), n_nn=t["n_nn"], nn_val=p(t["nn_val"]), actions=p(t["actions"]), n_frames=t["n_frames"],
                 last_end=t["last_end"], idx=p(d["idx"]), window=p(d["window_size"]), strategy=p(d["strategy"]), disp=p(d["disp"]),
                 noise=p(d["noise_step"]), u_choice=p(d["u_choice"]), u_rs=p(d["u_random_state"]), B=n, Tmax=T, A=7, min_window=8,
                 ids=p(ids), act=p(act), disp_out=p(dsp), window_size=p(ws), status=p(rp.status), stream=None)
        a.update(over)
        return list(a.values())

    fn = _lib.lib().tacorl_sample_play_windows
    EINVAL = -22  # TACORL_EINVAL (csrc/common.h)
    for k in ("B", "Tmax", "A", "n_items", "n_ep", "n_frames"):
        assert fn(*args(**{k: 0})) == EINVAL and fn(*args(**{k: -3})) == EINVAL, k
    assert fn(*args(n_nn=-1)) == EINVAL
    for mw in (0, -1, T + 1):
        assert fn(*args(min_window=mw)) == EINVAL, mw
    assert fn(*args(n_frames=T - 1, last_end=T - 2)) == EINVAL            # n_frames < Tmax
    assert fn(*args(last_end=-1)) == EINVAL and fn(*args(last_end=t["n_frames"])) == EINVAL
    required = ("lookup", "es", "ee", "actions", "idx", "window", "strategy", "disp", "u_choice", "u_rs", "ids", "act", "disp_out",
                "window_size", "status")
    for k in required + ("nn_ptr", "nn_val"):  # (the neighbour tables are required with n_nn > 0)
        assert fn(*args(**{k: None})) == EINVAL, k
    for k, tns in (("lookup", t["lookup"]), ("es", t["ep_start"]), ("ee", t["ep_end"]), ("nn_ptr", t["nn_ptr"]), ("nn_val", t["nn_val"]),
                   ("idx", d["idx"]), ("window", d["window_size"]), ("strategy", d["strategy"]), ("disp", d["disp"]),
                   ("noise", d["noise_step"]), ("u_choice", d["u_choice"]), ("u_rs", d["u_random_state"]), ("ids", ids),
                   ("disp_out", dsp), ("window_size", ws)):
        assert fn(*args(**{k: off(tns, 4)})) == EINVAL, k  # int64 / double tables need 8 bytes
    for k, tns in (("actions", t["actions"]), ("act", act), ("status", rp.status)):
        assert fn(*args(**{k: off(tns, 2)})) == EINVAL, k  # float / int need 4
    torch.cuda.synchronize()
    for x in (ids, dsp, ws):
        assert int(x.min()) == -7 and int(x.max()) == -7  # nothing ran
    assert float(act.min()) == -7.0 == float(act.max()) and int(rp.status.item()) == 0
    cur = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # NULL noise_step (no goal augmentation) and NULL neighbour tables with n_nn == 0 are accepted
    assert fn(*args(stream=cur, noise=None, nn_ptr=None, nn_val=None, n_nn=0)) == 0
    assert fn(*args(stream=cur)) == 0
    torch.cuda.synchronize()
    assert int(ids.min()) >= 0 and int(ids.max()) < t["n_frames"] and int(rp.status.item()) == 0
    assert int(ws.min()) >= 8 and int(ws.max()) <= 16 and torch.isfinite(act).all()


@pytest.mark.parametrize("min_ws,max_ws,goal_aug", [(8, 16, True), (16, 16, False)])
def test_device_draws_feed_the_kernel(min_ws, max_ws, goal_aug):
    """draw_device's tensors go to the kernel as they are; the host sampler on their copies gives the same batch."""
    ix = _index(min_ws, max_ws, goal_aug, "partial")
    d = ix.draw_device(1000, DEV, torch.Generator(device=DEV).manual_seed(5))
    assert all(t.is_cuda and t.shape == (1000,) for t in d.values())
    assert all(d[k].dtype == torch.int64 for k in ("idx", "window_size", "strategy", "disp", "noise_step"))
    assert d["u_choice"].dtype == torch.float64 and d["u_random_state"].dtype == torch.float64
    assert int(d["idx"].min()) >= 0 and int(d["idx"].max()) < len(ix) and int(d["disp"].min()) >= 1
    assert float(d["u_choice"].min()) >= 0.0 and float(d["u_choice"].max()) < 1.0 and float(d["u_random_state"].max()) < 1.0
    assert set(d["noise_step"].unique().tolist()) == ({-1, 0, 1} if goal_aug else {0})
    assert set(d["strategy"].unique().tolist()) == {0, 1}
    # the means of 1 000 draws, more than five standard errors wide: geometric(0.3) has mean 1 / 0.3 and standard deviation
    # sqrt(0.7) / 0.3 = 2.79 (standard error 0.088), the strategy is a fair coin (standard error 0.016)
    assert abs(float(d["disp"].double().mean()) - 1 / 0.3) < 0.5 and abs(float(d["strategy"].double().mean()) - 0.5) < 0.1
    if min_ws < max_ws:
        assert int(d["window_size"].min()) == min_ws and int(d["window_size"].max()) == max_ws
    got, s = _assert_equals_host(ix, _actions(7), d)
    assert (s["disp"] == -1).any() and (s["disp"] > 0).any()


# ---------------------------------------------------------------------------------------------- the replay and the step
_DATA = {}


def _dataset(hw=84, n=400):
    """tests/test_data_gpu.py::_dataset (400 uint8 frames, 7 actions with a +-1 gripper): built once per size, never written."""
    if (hw, n) not in _DATA:
        g = torch.Generator().manual_seed(3)
        frames = torch.randint(0, 256, (n, hw, hw, 3), dtype=torch.uint8, generator=g)
        acts = np.random.RandomState(4).uniform(-1, 1, size=(n, 7)).astype(np.float32)
        acts[:, -1] = np.where(acts[:, -1] >= 0, 1.0, -1.0)
        _DATA[hw, n] = (frames, acts)
    return _DATA[hw, n]


def test_dense_batch_equals_the_host_fed_replay():
    """HbmPlayReplay.batch(fused=False) against HbmReplay.batch(idx, draws, fused=False) on the same draws: the frames of each
    camera, the goal, actions, disp and window_size, bit for bit; the fused form carries the same id table."""
    from tacorl_amd.data.play_replay import HbmPlayReplay
    from tacorl_amd.data.replay import HbmReplay

    small, acts = _dataset(8, N)
    frames = {"rgb_static": small, "rgb_gripper": _dataset(16, N)[0]}
    ix = _index(8, 16, goal_aug=True, nn="partial")
    old = HbmReplay(frames, acts, ix, device=DEV)
    new = HbmPlayReplay(frames, acts, ix, device=DEV, batch_size=4)
    for n in (5, 33):
        d = _fresh_draws(ix, n, 50 + n)
        a = old.batch(d["idx"], d, fused=False)
        b = new.batch(d, fused=False)
        f = new.batch(d, fused=True)
        torch.cuda.synchronize()
        assert set(b) == set(a) - {"ready"} and "ready" not in f and set(f) == (set(b) - {"states", "goal"}) | {"replay"}
        for c in frames:
            assert b["states"][c].shape == (n, 16) + tuple(frames[c].shape[1:]) and b["states"][c].dtype == torch.uint8
            assert torch.equal(b["states"][c], a["states"][c]) and torch.equal(b["goal"][c], a["goal"][c]), c
            assert f["replay"]["frames"][c] is new.frames[c]
        assert torch.equal(b["actions"], a["actions"]) and torch.equal(b["disp"], a["disp"])
        for k in ("idx", "window_size"):  # device-resident here, host tensors there
            assert b[k].is_cuda and b[k].dtype == torch.int64 and torch.equal(b[k].cpu(), a[k]), k
        fa = old.batch(d["idx"], d, fused=True)
        torch.cuda.synchronize()
        assert torch.equal(f["replay"]["ids"], fa["replay"]["ids"]) and (f["replay"]["B"], f["replay"]["T"]) == (n, 16)
        assert torch.equal(f["actions"], b["actions"])
    new.check()
    nogoal = HbmPlayReplay(frames, acts, ix, device=DEV, include_goal=False).batch(d, fused=False)
    assert "goal" not in nogoal and "disp" not in nogoal and torch.equal(nogoal["states"]["rgb_static"], b["states"]["rgb_static"])


@pytest.mark.parametrize("fused", [True, False])
def test_a_batch_survives_the_batches_fetched_ahead(fused):
    """Hold `slots - 1` batches: the first is still intact; the one after them takes its buffers."""
    from tacorl_amd.data.play_replay import HbmPlayReplay

    frames, acts = _dataset(8, N)
    ix = _index(8, 16, nn="partial")
    slots = 4
    rp = HbmPlayReplay({"rgb_static": frames}, acts, ix, device=DEV, batch_size=6, slots=slots)
    g = torch.Generator(device=DEV).manual_seed(2)

    def tensors(b):
        t = {k: b[k] for k in ("actions", "disp", "idx", "window_size")}
        if fused:
            t["ids"] = b["replay"]["ids"]
        else:
            t.update(states=b["states"]["rgb_static"], goal=b["goal"]["rgb_static"])
        return t

    held = [rp.batch(ix.draw_device(6, DEV, g), fused=fused) for _ in range(slots - 1)]
    first = tensors(held[0])
    keep = {k: v.clone() for k, v in first.items()}
    assert len({tensors(b)["actions"].data_ptr() for b in held}) == slots - 1
    torch.cuda.synchronize()
    assert all(torch.equal(first[k], keep[k]) for k in keep)
    rp.batch(ix.draw_device(6, DEV, g), fused=fused)   # the slots-th batch: still another set
    torch.cuda.synchronize()
    assert all(torch.equal(first[k], keep[k]) for k in keep)
    again = tensors(rp.batch(ix.draw_device(6, DEV, g), fused=fused))  # ... and the one after it reuses the first's buffers
    torch.cuda.synchronize()
    assert again["actions"].data_ptr() == first["actions"].data_ptr() and not torch.equal(first["actions"], keep["actions"])
    # a larger batch than the ring was built for: the buffers are replaced and the allocation epoch moves
    from tacorl_amd import ops

    e0 = ops.alloc_epoch()
    big = rp.batch(ix.draw_device(40, DEV, g), fused=fused)
    assert big["actions"].shape == (40, 16, 7) and ops.alloc_epoch() > e0
    rp.check()


@pytest.mark.parametrize("min_ws,goal_aug", [(16, False), (8, True)])
def test_batch_path_does_not_synchronise_the_host(min_ws, goal_aug):
    """Draws, sampler and gathers are enqueued and nothing is read back: torch raises on a synchronising call in this mode."""
    from tacorl_amd.data.play_replay import HbmPlayReplay

    frames, acts = _dataset(8, N)
    ix = _index(min_ws, 16, goal_aug, "partial")
    rp = HbmPlayReplay({"rgb_static": frames}, acts, ix, device=DEV, batch_size=6)
    rp.batch(fused=False)  # (the dense form's gather buffers of the first slot exist now; the others are made below)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(len(rp._ring)):
            f, d = rp.batch(fused=True), rp.batch(fused=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert f["replay"]["ids"].is_cuda and d["states"]["rgb_static"].shape == (6, 16, 8, 8, 3)
    rp.check()


def _build(kind):
    import bench
    from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP
    from tests import cfg_util as K

    if kind == "playlmp":
        torch.manual_seed(3)
        strip = lambda c: {k: v for k, v in c.items() if k not in ("_target_", "_recursive_")}  # noqa: E731
        return PlayLMP(**strip(K.playlmp_cfg(device=DEV, compute_dtype="bf16", image_dtype="bf16")))
    torch.manual_seed(0)
    return bench.build_module(torch.device(DEV), "bf16", 16, 1, finetune=kind == "tacorl_finetune")


@pytest.mark.parametrize("augmented", [False, True])
@pytest.mark.parametrize("kind", ["tacorl", "tacorl_finetune", "playlmp"])
def test_steps_fed_by_the_three_replays_are_one_step(kind, augmented):
    """The geometry of tests/test_data_gpu.py::test_fused_replay_batch_equals_gathered_batch.  A step fed by
    HbmPlayReplay.batch(fused=True), one fed by its dense form and one fed by the parent's HbmReplay.batch(fused=True), on the
    same draws and the same augmentation tables: identical logs, identical stepped parameters."""
    from tacorl_amd.data.augment import AugmentSpec, draw_play_batch_augmentation
    from tacorl_amd.data.play_replay import HbmPlayReplay
    from tacorl_amd.data.replay import HbmReplay, PlayIndex

    frames, acts = _dataset()
    ix = PlayIndex([[0, 199], [200, 399]], 16, 16, goal_sampling_prob=0.3)
    rng = np.random.default_rng(1)
    B, T = 16, 16
    idx, draws = rng.integers(len(ix), size=B), ix.draw(B, rng)
    old = HbmReplay({"rgb_static": frames}, acts, ix, device=DEV)
    new = HbmPlayReplay({"rgb_static": frames}, acts, ix, device=DEV, batch_size=B)
    aug = None
    if augmented:
        aug = draw_play_batch_augmentation({"rgb_static": AugmentSpec(pad=4)}, B, T, DEV, torch.Generator(device=DEV).manual_seed(12))
    feeds = {"play_fused": lambda: new.batch(dict(draws, idx=idx), aug=aug, fused=True),
             "play_dense": lambda: new.batch(dict(draws, idx=idx), aug=aug, fused=False),
             "host_fused": lambda: old.batch(idx, draws, aug=aug, fused=True)}
    args = (0,) if kind == "playlmp" else ()
    logs, params = {}, {}
    for name, feed in feeds.items():
        m = _build(kind)
        b = feed()
        assert ("replay" in b) == (name != "play_dense") and ("aug" in b) == augmented
        torch.manual_seed(7); torch.cuda.manual_seed(7)
        m.training_step(b, *args)
        torch.cuda.synchronize()
        logs[name] = dict(m.logged)
        params[name] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ref = logs["host_fused"]
    assert ref and all(v == v for v in ref.values())
    for name in ("play_fused", "play_dense"):
        assert logs[name] == ref, (kind, augmented, name, logs[name], ref)
        assert params[name].keys() == params["host_fused"].keys()
        diff = [k for k, v in params[name].items() if not torch.equal(v, params["host_fused"][k])]
        assert not diff, (kind, augmented, name, diff[:5])
    new.check()


@pytest.mark.parametrize("form", ["fused", "dense"])
def test_trainer_fit_over_the_datamodule(form):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests", "fake_pl"), env.get("PYTHONPATH", "")])
    out = run_group([sys.executable, os.path.join(ROOT, "tests", "play_fit_script.py"), form], env, ROOT, timeout=300)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
