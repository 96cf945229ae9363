"""The resident D4RL window replay on the GPU: the sampler kernel (`tacorl_sample_d4rl_windows`) against the host
D4RLWindowIndex bit for bit (and, on the recorded draws, against the reference's items), HbmD4RLReplay's two batch forms, and
TACORL-D4RL / PlayLMP-D4RL steps fed by them - the host-assembled batch, the dense replay batch and the fused batch must be one
step: the same arithmetic on the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import d4rl_cfg as K
from tests.d4rl_window_util import VARIANTS, D4rlWindowGolden, synthetic_dataset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = D4rlWindowGolden()
GUARD = 8
_DATA = {}


def _dataset(S=29, A=8):
    """The synthetic dataset at (S, A): built once per shape, never written ((29, 8) is the fixture's)."""
    if (S, A) not in _DATA:
        _DATA[S, A] = synthetic_dataset(S=S, A=A)
    return _DATA[S, A]


def _index(data, **kw):
    from tacorl_amd.data.d4rl_replay import D4RLWindowIndex

    return D4RLWindowIndex(data["timeouts"], data["terminals"], **kw)


def _replay(data, ix, **kw):
    from tacorl_amd.data.d4rl_replay import HbmD4RLReplay

    return HbmD4RLReplay(data["observations"], data["actions"], ix, device=DEV, **kw)


def _guarded(n, dtype):
    """n elements prefilled with NaN (int64: -7) and GUARD elements behind them that nothing may touch."""
    t = torch.full((n + GUARD,), float("nan") if dtype == torch.float32 else -7, dtype=dtype, device=DEV)
    t[n:] = 12345
    return t


def _kernel(rp, draws):
    """One sampler launch into guarded buffers; every element written, no guard touched.  Returns numpy outputs."""
    from tacorl_amd import ops

    d = rp._draws(draws)
    B, T, S, A, Gd = int(d["idx"].numel()), rp.T, rp.S, rp.A, rp.G
    sizes = {"obs": B * T * S, "act": B * T * A, "goal": B * Gd, "reached": B, "done": B, "window_size": B, "ids": 2 * B}
    buf = {k: _guarded(n, torch.int64 if k in ("window_size", "ids") else torch.float32) for k, n in sizes.items()}
    v = {k: buf[k][:n] for k, n in sizes.items()}
    goal = dict(goal=v["goal"], reached=v["reached"], done=v["done"]) if Gd else {}
    ops.sample_d4rl_windows(rp.tables, d, T, Gd, rp.index.min, rp.index.goal_threshold, v["obs"], v["act"], rp.status,
                            window_size=v["window_size"], ids=v["ids"], **goal)
    torch.cuda.synchronize()
    out = {}
    for k, n in sizes.items():
        assert bool((buf[k][n:] == 12345).all()), f"{k}: a guard element was written"
        if Gd or k not in ("goal", "reached", "done"):
            t = buf[k][:n]
            assert not bool(torch.isnan(t).any() if t.is_floating_point() else (t == -7).any()), f"{k}: an element was not written"
            out[k] = t.cpu().numpy()
    return out, (B, T, S, A, Gd)


def _assert_equals_host(rp, data, draws):
    ix = rp.index
    out, (B, T, S, A, Gd) = _kernel(rp, draws)
    s = ix.sample(None, {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in draws.items()}, data["observations"],
                  data["actions"])
    assert np.array_equal(out["obs"].reshape(B, T, S), s["observations"])
    assert np.array_equal(out["act"].reshape(B, T, A), s["actions"])
    assert np.array_equal(out["window_size"], s["window"]) and np.array_equal(out["ids"][:B], s["start"])
    if Gd:
        assert np.array_equal(out["ids"][B:], s["goal_step"])
        assert np.array_equal(out["goal"].reshape(B, Gd), s["goal"])
        assert np.array_equal(out["reached"], s["goal_reached"].astype(np.float32)) and np.array_equal(out["done"], out["reached"])
    assert int(rp.status.item()) == 0
    rp.check()
    return s


# ------------------------------------------------------------------------------------------------ kernel against host
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_kernel_equals_host_sampler_and_the_reference_on_the_recorded_draws(variant):
    ix, v = G.index(variant), G.variants[variant]
    s = _assert_equals_host(_replay(G.dataset, ix), G.dataset, G.draws(variant))
    assert np.array_equal(s["observations"], v["observations"]) and np.array_equal(s["actions"], v["actions"])
    if VARIANTS[variant]["include_goal"]:
        assert np.array_equal(s["goal"], v["goal"]) and np.array_equal(s["goal_reached"], v["goal_reached"])


@pytest.mark.parametrize("B", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("S,A,goal", [(29, 8, True), (29, 8, False), (5, 3, True)])
def test_kernel_equals_host_sampler_on_fresh_draws(B, S, A, goal):
    """One wavefront per window, four per block: a part block, three of four, a full block, a block tail, many blocks."""
    data = _dataset(S, A)
    for mn, mx in ((8, 8), (8, 16), (2, 3)):
        ix = _index(data, min_window_size=mn, max_window_size=mx, include_goal=goal)
        d = ix.draw(B, np.random.default_rng(1000 * B + 10 * mx + S))
        if goal:
            d["disp"][::2][:3] = 2 ** 62  # a huge draw in a few slots: the episode end, no overflow
        s = _assert_equals_host(_replay(data, ix), data, d)
        if goal:
            assert np.array_equal(s["goal_step"][::2][:3], ix.episode_end(s["start"])[::2][:3])
        if B == 257:
            assert set(d["window"]) == set(range(mn, mx + 1))
            if goal:
                assert s["goal_reached"].any() and not s["goal_reached"].all()


def test_device_draws_feed_the_kernel():
    """draw_device's tensors go to the kernel as they are; the host sampler on their copies gives the same batch."""
    ix = G.index("tacorl_8_16")
    d = ix.draw_device(1000, DEV, torch.Generator(device=DEV).manual_seed(5))
    assert set(d) == {"idx", "window", "disp"} and all(t.is_cuda and t.dtype == torch.int64 for t in d.values())
    assert int(d["disp"].min()) >= 1 and int(d["idx"].min()) >= 0 and int(d["idx"].max()) < len(ix)
    assert set(d["window"].tolist()) == set(range(8, 17))
    _assert_equals_host(_replay(G.dataset, ix), G.dataset, d)


def test_entry_point_refuses_bad_arguments_without_launching():
    from tacorl_amd import _lib

    ix = G.index("tacorl_8_16")
    rp = _replay(G.dataset, ix)
    t, n, T, S, A = rp.tables, 8, 16, 29, 8
    d = ix.draw_device(n, DEV, torch.Generator(device=DEV).manual_seed(0))
    outs = {k: torch.full((m,), -7.0, device=DEV) for k, m in (("obs", n * T * S), ("act", n * T * A), ("goal", n * 2), ("reached", n),
                                                              ("done", n))}
    ints = {"ws": torch.full((n,), -7, dtype=torch.int64, device=DEV), "ids": torch.full((2 * n,), -7, dtype=torch.int64, device=DEV)}
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def args(**over):
        a = dict(lookup=p(t["lookup"]), n_items=t["lookup"].numel(), es=p(t["ep_start"]), ee=p(t["ep_end"]), n_ep=t["ep_start"].numel(),
                 observations=p(t["observations"]), actions=p(t["actions"]), n_frames=t["n_frames"], idx=p(d["idx"]),
                 window=p(d["window"]), disp=p(d["disp"]), B=n, Tmax=T, S=S, A=A, G=2, min_window=8, threshold=0.5, obs=p(outs["obs"]),
                 act=p(outs["act"]), goal=p(outs["goal"]), reached=p(outs["reached"]), done=p(outs["done"]), ws=p(ints["ws"]),
                 ids=p(ints["ids"]), status=p(rp.status), stream=None)
        a.update(over)
        return list(a.values())

    fn = _lib.lib().tacorl_sample_d4rl_windows
    assert fn(*args(B=0)) != 0 and fn(*args(B=-3)) != 0 and fn(*args(Tmax=0)) != 0 and fn(*args(S=0)) != 0 and fn(*args(A=-1)) != 0
    assert fn(*args(G=1)) != 0 and fn(*args(G=30)) != 0 and fn(*args(min_window=0)) != 0 and fn(*args(min_window=17)) != 0
    assert fn(*args(n_items=0)) != 0 and fn(*args(n_ep=0)) != 0 and fn(*args(n_frames=15)) != 0
    for k in ("lookup", "es", "ee", "observations", "actions", "idx", "window", "disp", "obs", "act", "status"):
        assert fn(*args(**{k: None})) != 0, k
    assert fn(*args(idx=C.c_void_p(d["idx"].data_ptr() + 4))) != 0  # a misaligned int64 table
    assert fn(*args(obs=C.c_void_p(outs["obs"].data_ptr() + 2))) != 0 and fn(*args(ids=C.c_void_p(ints["ids"].data_ptr() + 4))) != 0
    torch.cuda.synchronize()
    assert all(float(o.min()) == -7.0 == float(o.max()) for o in outs.values())  # nothing ran
    assert all(int(o.min()) == -7 == int(o.max()) for o in ints.values()) and int(rp.status.item()) == 0
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert fn(*args(stream=stream)) == 0
    assert fn(*args(stream=stream, goal=None, reached=None, done=None, ws=None, ids=None)) == 0  # the optional outputs
    torch.cuda.synchronize()
    s = ix.sample(None, {k: v.cpu().numpy() for k, v in d.items()}, G.dataset["observations"], G.dataset["actions"])
    assert np.array_equal(outs["obs"].cpu().numpy().reshape(n, T, S), s["observations"])
    assert np.array_equal(ints["ids"].cpu().numpy(), np.concatenate([s["start"], s["goal_step"]])) and int(rp.status.item()) == 0


def test_out_of_range_draws_are_clamped_and_raise_the_status_word():
    """One idx == len(index) and one window == Tmax + 1 among valid draws.  The clamp precedes every table access: this
    exercises the clamp, not a fault."""
    ix = G.index("tacorl_8_16")
    rp = _replay(G.dataset, ix)
    d = ix.draw(12, np.random.default_rng(7))
    good, _ = _kernel(rp, d)
    rp.check()
    bad = {k: v.copy() for k, v in d.items()}
    bad["idx"][3], bad["window"][9] = len(ix), ix.max + 1
    out, (B, T, S, A, Gd) = _kernel(rp, bad)
    assert int(rp.status.item()) == 1
    with pytest.raises(IndexError):
        rp.check()
    assert out["ids"].min() >= 0 and out["ids"].max() < ix.n_frames
    assert out["ids"][3] == ix.episode_lookup[-1] and out["window_size"][9] == ix.max
    assert out["window_size"].min() >= ix.min and out["window_size"].max() <= ix.max
    rows = np.array([b for b in range(B) if b not in (3, 9)])
    for k, w in (("obs", T * S), ("act", T * A), ("goal", Gd), ("reached", 1), ("done", 1), ("window_size", 1)):
        assert np.array_equal(out[k].reshape(B, w)[rows], good[k].reshape(B, w)[rows]), k
    assert np.array_equal(out["ids"].reshape(2, B)[:, rows], good["ids"].reshape(2, B)[:, rows])


# -------------------------------------------------------------------------------------------------- the replay's forms
def test_dense_batch_has_the_reference_schema():
    for variant in ("tacorl_8_16", "lmp_8_16"):
        ix = G.index(variant)
        rp = _replay(G.dataset, ix, batch_size=4)
        d = G.draws(variant)
        b = rp.batch(d, fused=False)
        torch.cuda.synchronize()
        goal = VARIANTS[variant]["include_goal"]
        assert set(b) == {"observations", "actions", "idx", "window_size"} | ({"goal", "goal_reached"} if goal else set())
        v = G.variants[variant]
        assert b["observations"].shape == (64, 16, 29) and b["actions"].shape == (64, 16, 8)
        assert b["idx"].dtype == b["window_size"].dtype == torch.int64 and b["observations"].dtype == torch.float32
        assert np.array_equal(b["observations"].cpu().numpy(), v["observations"]) and np.array_equal(b["actions"].cpu().numpy(), v["actions"])
        assert np.array_equal(b["idx"].cpu().numpy(), v["idx"]) and np.array_equal(b["window_size"].cpu().numpy(), v["window"])
        if goal:
            assert b["goal"].shape == (64, 2) and b["goal_reached"].shape == (64,)
            assert np.array_equal(b["goal"].cpu().numpy(), v["goal"])
            assert np.array_equal(b["goal_reached"].cpu().numpy(), v["goal_reached"].astype(np.float32))
        f = rp.batch(d, fused=True)
        assert set(f) == {"replay"} and f["replay"]["kind"] == "d4rl_window" and f["replay"]["replay"] is rp
        assert f["replay"]["B"] == 64 and f["replay"]["T"] == 16 and set(f["replay"]["draws"]) == {"idx", "window", "disp"}
        rp.check()


def test_batches_survive_a_trainer_that_fetches_ahead():
    """The dense buffers are a ring: with slots=3 the first batch is intact after two more draws; the third overwrites it."""
    ix = G.index("tacorl_8_16")
    rp = _replay(G.dataset, ix, batch_size=8, slots=3)
    gen = torch.Generator(device=DEV).manual_seed(51)
    keys = ("observations", "actions", "goal", "goal_reached", "window_size")
    first = rp.batch(ix.draw_device(8, DEV, gen), fused=False)
    keep = {k: first[k].clone() for k in keys}
    later = [rp.batch(ix.draw_device(8, DEV, gen), fused=False) for _ in range(2)]
    torch.cuda.synchronize()
    assert all(torch.equal(first[k], keep[k]) for k in keys)
    assert all(not torch.equal(b["observations"], keep["observations"]) for b in later)
    assert first["observations"].data_ptr() not in {b["observations"].data_ptr() for b in later}
    again = rp.batch(ix.draw_device(8, DEV, gen), fused=False)  # the fourth draw of a ring of three reuses the first slot
    torch.cuda.synchronize()
    assert again["observations"].data_ptr() == first["observations"].data_ptr()
    assert not torch.equal(first["observations"], keep["observations"])
    rp.check()


# ------------------------------------------------------------------------------------------------------------ the steps
def _seeded(build):
    torch.manual_seed(3); torch.cuda.manual_seed(3)
    return build()


def _tacorl():
    lmp = K.build(K.playlmp_d4rl_cfg(latent=16, T=8, device=DEV, compute_dtype="f32"))
    return K.build(K.tacorl_d4rl_cfg(play_lmp=lmp, finetune_action_decoder=True, device=DEV, compute_dtype="f32"))


def _three_forms(rp, d, data, goal):
    s = rp.index.sample(None, d, data["observations"], data["actions"])
    host = {"observations": torch.from_numpy(s["observations"]), "actions": torch.from_numpy(s["actions"]),
            "idx": torch.from_numpy(s["idx"]), "window_size": torch.from_numpy(s["window"])}
    if goal:
        host.update(goal=torch.from_numpy(s["goal"]), goal_reached=torch.from_numpy(s["goal_reached"]))
    return {"host": lambda: host, "dense": lambda: rp.batch(d, fused=False), "fused": lambda: rp.batch(d, fused=True)}


def _draws_with_both_flags(ix, data, B):
    for seed in range(200):
        d = ix.draw(B, np.random.default_rng(seed))
        r = ix.sample(None, d, data["observations"], data["actions"])["goal_reached"]
        if 0 < r.sum() < B:
            return d
    raise AssertionError("no draw with both values of goal_reached")


def _run(build, forms, noises, plan_of, steps=2):
    """`steps` training steps per form on modules of equal parameters; logged scalars, plan and parameters per form."""
    res = {}
    for name, make in forms.items():
        mod = _seeded(build)
        logs = []
        for step in range(steps):
            mod.logged = {}
            mod.training_step(make[step](), 0, noise={k: v.to(DEV) for k, v in noises[step].items()})
            torch.cuda.synchronize()
            assert mod.logged and all(np.isfinite(v) for v in mod.logged.values()), mod.logged
            logs.append(dict(mod.logged))
        res[name] = (logs, plan_of(mod).clone(), {k: v.clone() for k, v in mod.state_dict().items()}, mod)
    return res


def _assert_one_step(res):
    (l0, p0, s0, _), names = res["host"], [n for n in res if n != "host"]
    for n in names:
        logs, plan, sd, _ = res[n]
        assert logs == l0, (n, logs, l0)
        assert torch.equal(plan, p0), n
        assert set(sd) == set(s0) and all(torch.equal(sd[k], s0[k]) for k in s0), (n, [k for k in s0 if not torch.equal(sd[k], s0[k])])


def test_tacorl_d4rl_steps_are_the_same_from_all_three_batch_forms():
    g = K.D4rlGolden("tacorl_d4rl_ad")  # (its recorded noise: B = 3, latent plan 16, n = 4)
    data = G.dataset
    ix = G.index("tacorl_8_8")
    rp = _replay(data, ix, batch_size=3)
    ds = [_draws_with_both_flags(ix, data, 3), ix.draw(3, np.random.default_rng(77))]
    per_step = [_three_forms(rp, d, data, True) for d in ds]
    forms = {n: [f[n] for f in per_step] for n in ("host", "dense", "fused")}
    res = _run(_tacorl, forms, [g.noise(0), g.noise(1)], lambda m: m.engine.action)
    _assert_one_step(res)
    l0, _, s0, mod = res["fused"]
    assert l0[0] != l0[1] and "train/action_loss" in l0[0]
    # the fused staging wrote the step's own buffers
    s = ix.sample(None, ds[1], data["observations"], data["actions"])
    assert np.array_equal(mod.engine.obs.cpu().numpy(), s["observations"]) and np.array_equal(mod._acts.cpu().numpy(), s["actions"])
    assert np.array_equal(mod.engine.goal.cpu().numpy(), s["goal"])
    assert np.array_equal(mod.engine.reward.cpu().numpy(), s["goal_reached"].astype(np.float32))
    assert torch.equal(mod.engine.done, mod.engine.reward)
    # validation on the fused form moves nothing
    mod.logged = {}
    mod.validation_step(rp.batch(ds[0], fused=True), 0, noise={k: v.to(DEV) for k, v in g.noise(0).items()})
    torch.cuda.synchronize()
    assert mod.logged and all(k.startswith("validation/") and np.isfinite(v) for k, v in mod.logged.items())
    assert all(torch.equal(v, s0[k]) for k, v in mod.state_dict().items())
    rp.check()


@pytest.mark.parametrize("T,mn", [(8, 8), (16, 8)])
def test_playlmp_d4rl_steps_are_the_same_from_all_three_batch_forms(T, mn):
    data = G.dataset
    ix = _index(data, min_window_size=mn, max_window_size=T)  # no goal
    rp = _replay(data, ix, batch_size=3)
    ds = [ix.draw(3, np.random.default_rng(80 + T + k)) for k in range(2)]
    if T == 16:
        assert len(set(ds[0]["window"]) | set(ds[1]["window"])) > 1 and min(ds[0]["window"].min(), ds[1]["window"].min()) < 16
    per_step = [_three_forms(rp, d, data, False) for d in ds]
    forms = {n: [f[n] for f in per_step] for n in ("host", "dense", "fused")}
    gen = torch.Generator().manual_seed(9)
    noises = [dict(eps_plan=torch.randn(3, 16, generator=gen), u_plan=torch.rand(3, 16, generator=gen)) for _ in range(2)]
    build = lambda: K.build(K.playlmp_d4rl_cfg(latent=16, T=T, device=DEV, compute_dtype="f32", dropout_p=0.0))  # noqa: E731
    res = _run(build, forms, noises, lambda m: m.plan)
    _assert_one_step(res)
    mod = res["fused"][3]
    s = ix.sample(None, ds[1], data["observations"], data["actions"])
    assert np.array_equal(mod.obs.cpu().numpy(), s["observations"]) and np.array_equal(mod.acts.cpu().numpy(), s["actions"])
    assert np.array_equal(mod.goal.cpu().numpy(), s["observations"][:, -1, :2])
    with pytest.raises(ValueError):  # no goal in this index: nothing to write a goal from
        rp.sample_into(rp._draws(ds[0]), mod.obs, mod.acts, goal=mod.goal)
    if T == 8:
        with pytest.raises(ValueError):  # ... and TACORL cannot be staged from it
            _seeded(_tacorl).training_step(rp.batch(ds[0], fused=True), 0)
    rp.check()


@pytest.mark.parametrize("fused", [True, False])
def test_trainer_fit_over_the_datamodule(fused, tmp_path):
    from tacorl_amd import lightning as L
    from tacorl_amd.data.d4rl_replay import D4RLDataModule, D4RLWindowLoader

    np.savez(tmp_path / "antmaze.npz", **G.dataset)
    dataset = {"path": str(tmp_path / "antmaze.npz"), "min_window_size": 8, "max_window_size": 8, "include_goal": True,
               "goal_sampling_prob": 0.3, "d4rl_env": K.ENV}
    dm = D4RLDataModule(dataset, batch_size=3, steps_per_epoch=3, num_workers=4, pin_memory=True, device=DEV, fused=fused,
                        generator=torch.Generator(device=DEV).manual_seed(41))
    dm.setup()
    loader = dm.train_dataloader()
    assert isinstance(loader, D4RLWindowLoader) and len(loader) == 3 and len(dm.index) == 110
    assert D4RLDataModule(dict(dataset), batch_size=3, device=DEV).train_dataloader().steps_per_epoch == 110 // 3
    m = _seeded(_tacorl)
    tr = L.MiniTrainer(max_epochs=2, log_every_n_steps=1)
    tr.fit(m, datamodule=dm)
    torch.cuda.synchronize()
    assert tr.global_step == 6 and tr.current_epoch == 2
    assert m.logged and all(np.isfinite(v) for v in m.logged.values())
    assert np.isfinite(tr.logged_metrics["train/q1_loss"]) and np.isfinite(tr.logged_metrics["train/action_loss"])
    dm.replay.check()
