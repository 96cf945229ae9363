"""The resident transition replay on the GPU: the sampler kernel (`tacorl_sample_transitions`) against the host
TransitionIndex bit for bit, HbmTransitionReplay's two batch forms, and CQL_Offline steps fed by them - the fused batch
(frames read by id out of the dataset), the gathered uint8 batch and the host-transformed fp32 batch must be one step."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.transition_util import TransitionGolden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = TransitionGolden()
N, HW, B = 200, 84, 8
EP = [[0, 49], [50, 129], [130, 199]]  # three episodes of unequal length


def _all_strategies(ep, n_frames, nn, **kw):
    from tacorl_amd.data.replay import STRATEGIES, TransitionIndex

    return TransitionIndex(ep, n_frames=n_frames, goal_strategy_prob={k: 1 / 6 for k in STRATEGIES}, nn_steps_from_step=nn, **kw)


def _sampled(ix, actions, draws):
    """(replay, its fused batch) for the draws, with nothing but the tables resident (no camera)."""
    from tacorl_amd.data.replay import HbmTransitionReplay

    rp = HbmTransitionReplay({}, actions, ix, device=DEV, batch_size=8)
    b = rp.batch(draws, fused=True)
    torch.cuda.synchronize()
    return rp, b


def _assert_equals_host(ix, actions, draws):
    s = ix.sample(None, draws)
    rp, b = _sampled(ix, actions, draws)
    n = len(s["step"])
    ids = b["replay"]["ids"].cpu().numpy()
    assert ids.shape == (3, n) and b["replay"]["B"] == n and b["replay"]["kind"] == "transition"
    assert np.array_equal(ids, np.stack([s["step"], s["next"], s["goal"]]))
    assert np.array_equal(b["rewards"].cpu().numpy(), s["reward"].astype(np.float32))
    assert np.array_equal(b["terminals"].cpu().numpy(), s["done"].astype(np.float32))
    assert np.array_equal(b["actions"].cpu().numpy(), np.asarray(actions, np.float32)[s["step"]])
    assert int(rp.status.item()) == 0
    rp.check()
    return s


@pytest.mark.parametrize("variant", list(G.variants))
def test_kernel_equals_host_sampler_on_the_recorded_draws(variant):
    ix = G.index(variant)
    s = _assert_equals_host(ix, G.actions, G.draws(variant, ix))
    assert np.array_equal(s["goal"], G.variants[variant]["goal"])  # ... which are the reference dataset's items


@pytest.mark.parametrize("n", [1, 7, 256, 1000])
def test_kernel_equals_host_sampler_on_fresh_draws(n):
    """One thread per sample in 256-thread blocks: one item, a partial block, a full block, a block tail."""
    ix = _all_strategies(G.ep, G.cfg["n_frames"], G.nn, initial_horizon=5)
    d = ix.draw(n, np.random.default_rng(100 + n))
    if n >= 256:
        assert sorted(set(d["strategy"])) == list(range(6))
    _assert_equals_host(ix, G.actions, d)
    # ... and with a horizon longer than any episode, and without any neighbour table (similar -> random)
    ix2 = _all_strategies(G.ep, G.cfg["n_frames"], None, initial_horizon=100)
    _assert_equals_host(ix2, G.actions, d)


def test_device_draws_feed_the_kernel():
    """draw_device's tensors go to the kernel as they are; the host sampler on their copies gives the same batch."""
    ix = _all_strategies(G.ep, G.cfg["n_frames"], G.nn)
    d = ix.draw_device(1000, DEV, torch.Generator(device=DEV).manual_seed(5))
    assert all(t.is_cuda for t in d.values()) and sorted(set(d["strategy"].tolist())) == list(range(6))
    assert int(d["disp"].min()) >= 1 and float(d["u_choice"].max()) < 1.0 and int(d["idx"].max()) < len(ix)
    s = ix.sample(None, {k: v.cpu().numpy() for k, v in d.items()})
    rp, b = _sampled(ix, G.actions, d)
    assert np.array_equal(b["replay"]["ids"].cpu().numpy(), np.stack([s["step"], s["next"], s["goal"]]))
    rp.check()


def test_entry_point_refuses_bad_arguments_without_launching():
    from tacorl_amd import _lib
    from tacorl_amd.data.replay import HbmTransitionReplay

    ix = G.index("geo_sim")
    rp = HbmTransitionReplay({}, G.actions, ix, device=DEV, batch_size=8)
    t, n = rp.tables, 8
    d = ix.draw_device(n, DEV, torch.Generator(device=DEV).manual_seed(0))
    ids = torch.full((3, n), -7, dtype=torch.int64, device=DEV)
    out = [torch.full((n, 7), -7.0, device=DEV), torch.full((n,), -7.0, device=DEV), torch.full((n,), -7.0, device=DEV)]
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def args(**over):
        a = dict(steps=p(t["steps"]), n_steps=t["steps"].numel(), es=p(t["ep_start"]), ee=p(t["ep_end"]), n_ep=t["ep_start"].numel(),
                 nn_ptr=p(t["nn_ptr"]), n_nn=t["n_nn"], nn_val=p(t["nn_val"]), actions=p(t["actions"]), idx=p(d["idx"]),
                 strategy=p(d["strategy"]), disp=p(d["disp"]), u=p(d["u_choice"]), horizon=8, n_frames=t["n_frames"], B=n, A=7,
                 ids=p(ids), action=p(out[0]), reward=p(out[1]), done=p(out[2]), status=p(rp.status), stream=None)
        a.update(over)
        return list(a.values())

    fn = _lib.lib().tacorl_sample_transitions
    assert fn(*args(B=0)) != 0 and fn(*args(B=-3)) != 0 and fn(*args(A=0)) != 0
    assert fn(*args(steps=None)) != 0 and fn(*args(es=None)) != 0 and fn(*args(actions=None)) != 0 and fn(*args(ids=None)) != 0
    assert fn(*args(nn_val=None)) != 0 and fn(*args(status=None)) != 0
    assert fn(*args(idx=C.c_void_p(d["idx"].data_ptr() + 4))) != 0  # misaligned int64 table
    torch.cuda.synchronize()
    assert int(ids.min()) == -7 and int(ids.max()) == -7 and all(float(o.min()) == -7.0 == float(o.max()) for o in out)  # nothing ran
    assert fn(*args(stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))) == 0
    torch.cuda.synchronize()
    assert int(ids.min()) >= 0 and int(ids.max()) < t["n_frames"] and int(rp.status.item()) == 0


# ---------------------------------------------------------------------------------------------- the replay and the step
_DATA = {}


def _dataset():
    """200 uint8 frames of two cameras, actions, neighbour lists: built once, never written."""
    if not _DATA:
        g = torch.Generator().manual_seed(3)
        _DATA["frames"] = {"rgb_static": torch.randint(0, 256, (N, HW, HW, 3), dtype=torch.uint8, generator=g).to(DEV),
                           "rgb_gripper": torch.randint(0, 256, (N, 64, 64, 3), dtype=torch.uint8, generator=g).to(DEV)}
        acts = np.random.RandomState(4).uniform(-1, 1, size=(N, 7)).astype(np.float32)
        acts[:, -1] = np.where(acts[:, -1] >= 0, 1.0, -1.0)
        _DATA["actions"] = acts
        _DATA["nn"] = {s: [int(x) for x in np.random.RandomState(s).randint(0, N, size=s % 4)] for s in range(N)}
    return _DATA["frames"], _DATA["actions"], _DATA["nn"]


def _replay(cams=("rgb_static",)):
    from tacorl_amd.data.replay import HbmTransitionReplay

    frames, acts, nn = _dataset()
    ix = _all_strategies(EP, N, nn)
    return HbmTransitionReplay({c: frames[c] for c in cams}, acts, ix, device=DEV, batch_size=B), ix


def _module(compute):
    from tacorl_amd.lightning import instantiate
    from tests import cfg_util

    torch.manual_seed(3); torch.cuda.manual_seed(3)
    return instantiate(cfg_util.cql_cfg(device=DEV, compute_dtype=compute, image_dtype=compute))


def _step(mod, batch, fn="training_step"):
    torch.manual_seed(7); torch.cuda.manual_seed(7)  # the step's own noise
    getattr(mod, fn)(batch)
    torch.cuda.synchronize()
    out = dict(mod.logged)
    assert out and all(np.isfinite(v) for v in out.values()), out
    return out


def _clone(b):
    return {k: _clone(v) if isinstance(v, dict) else (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}


def _host_fp32(frames, ids, small, obs_cams, goal_cams):
    """The reference pipeline on the host: frames[ids] -> ToTensor -> Normalize(0.5, 0.5), NCHW fp32, computed by the CPU
    (a true division by 255, as the pack kernel's; torch's device kernels multiply by the reciprocal) and then moved."""
    hid = ids.cpu()
    t = lambda c, k: (((frames[c].cpu()[hid[k]].permute(0, 3, 1, 2).contiguous().float() / 255.0) - 0.5) / 0.5).to(DEV)  # noqa: E731
    goal = {c: t(c, 2) for c in goal_cams}
    return {"observations": {"observation": {c: t(c, 0) for c in obs_cams}, "goal": goal},
            "next_observations": {"observation": {c: t(c, 1) for c in obs_cams}, "goal": goal},
            "actions": small["actions"].clone(), "rewards": small["rewards"].clone(), "terminals": small["terminals"].clone()}


def test_gathered_batch_has_the_reference_schema():
    rp, ix = _replay(("rgb_static", "rgb_gripper"))
    d = ix.draw(B, np.random.default_rng(2))
    s = ix.sample(None, d)
    b = rp.batch(d, fused=False)
    torch.cuda.synchronize()
    assert set(b) == {"observations", "next_observations", "actions", "rewards", "terminals"}
    assert set(b["observations"]) == set(b["next_observations"]) == {"observation", "goal"}
    frames, acts, _ = _dataset()
    for c in ("rgb_static", "rgb_gripper"):
        for got, k in ((b["observations"]["observation"][c], "step"), (b["next_observations"]["observation"][c], "next"),
                       (b["observations"]["goal"][c], "goal"), (b["next_observations"]["goal"][c], "goal")):
            assert got.dtype == torch.uint8 and torch.equal(got, frames[c][torch.from_numpy(s[k]).to(DEV)]), (c, k)
    assert np.array_equal(b["actions"].cpu().numpy(), acts[s["step"]])
    assert np.array_equal(b["rewards"].cpu().numpy(), s["reward"].astype(np.float32))
    rp.check()


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_cql_step_is_the_same_from_all_three_batch_forms(compute):
    rp, ix = _replay()
    frames = _dataset()[0]
    d = ix.draw(B, np.random.default_rng(11))
    assert len(set(d["strategy"])) >= 3 and 0 < ix.sample(None, d)["reward"].sum() < B
    outs, grads = [], []
    for form in ("fused", "gathered", "host"):
        b = rp.batch(d, fused=form != "gathered")
        if form == "host":
            b = _host_fp32(frames, b["replay"]["ids"], b, ["rgb_static"], ["rgb_static"])
        m = _module(compute)
        outs.append(_step(m, b))
        grads.append({k: v.clone() for k, v in m.named_gradients().items()})
    assert outs[0] == outs[1] == outs[2], outs
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]) and torch.equal(grads[0][k], grads[2][k]), k
    rp.check()


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_goal_frames_are_read_from_goal_cameras_only(compute):
    """Observation camera rgb_static (84x84), goal camera rgb_gripper (64x64), the three batch forms again: the fused step
    packs obs / next out of the first dataset and the goal out of the second, and equals - scalars and gradients - the
    steps of the gathered uint8 batch and of a host-transformed batch that carries nothing but those images."""
    from tests import goalcams_util as GC

    obs_cams, goal_cams = ["rgb_static"], ["rgb_gripper"]
    rp, ix = _replay(("rgb_static", "rgb_gripper"))
    frames = _dataset()[0]
    d = ix.draw(B, np.random.default_rng(12))
    outs, grads = [], []
    for form in ("fused", "gathered", "host"):
        b = rp.batch(d, fused=form != "gathered")
        if form == "host":
            b = _host_fp32(frames, b["replay"]["ids"], b, obs_cams, goal_cams)
        torch.manual_seed(3); torch.cuda.manual_seed(3)
        m = GC.build(obs_cams, goal_cams, compute=compute)
        outs.append(_step(m, b))
        grads.append({k: v.clone() for k, v in m.named_gradients().items()})
        if form == "fused":
            e = m.engine
            hid = b["replay"]["ids"].cpu()
            # NHWC, as the image buffers; bf16 images are the rounded f32 values
            norm = lambda c, k: (((frames[c].cpu()[hid[k]].float() / 255.0) - 0.5) / 0.5).to(e.X3[c].dtype)  # noqa: E731
            assert list(e.slot["rgb_static"]) == ["obs", "next"] and list(e.slot["rgb_gripper"]) == ["goal"]
            assert torch.equal(e.X3["rgb_static"].cpu(), torch.cat([norm("rgb_static", 0), norm("rgb_static", 1)]))
            assert torch.equal(e.X3["rgb_gripper"].cpu(), norm("rgb_gripper", 2))
    assert outs[0] == outs[1] == outs[2], outs
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]) and torch.equal(grads[0][k], grads[2][k]), k
    rp.check()


def test_augmented_step_fused_equals_gathered():
    from tacorl_amd.data.augment import AugmentSpec, draw_transition_batch_augmentation

    rp, ix = _replay()
    d = ix.draw(B, np.random.default_rng(13))
    aug = draw_transition_batch_augmentation({"rgb_static": AugmentSpec(pad=4)}, B, DEV, torch.Generator(device=DEV).manual_seed(14))
    outs = []
    for fused in (True, False, True):
        b = rp.batch(d, aug=aug, fused=fused)
        assert b["aug"] is aug
        outs.append(_step(_module("bf16"), b))
    plain = _step(_module("bf16"), rp.batch(d, fused=True))
    assert outs[0] == outs[1], outs          # fused route = gathered route for the same tables
    assert outs[0] == outs[2]                # reproducible
    assert outs[0] != plain                  # ... and the tables were applied
    # a resizing spec sets the encoders' geometry: 84x84 frames -> 64x64 images
    aug = draw_transition_batch_augmentation({"rgb_static": AugmentSpec(pad=4, resize=(64, 64))}, B, DEV,
                                             torch.Generator(device=DEV).manual_seed(15))
    rs = []
    for fused in (True, False):
        m = _module("bf16")
        rs.append(_step(m, rp.batch(d, aug=aug, fused=fused)))
        assert tuple(m.engine.X3["rgb_static"].shape[1:3]) == (64, 64)
    assert rs[0] == rs[1]
    rp.check()


def test_training_steps_under_graph_replay_equal_ordinary_batches():
    """Fresh device draws per step, both modules with enable_graph(): module A takes the fused replay batches (the eager
    pack refills the image slots and the transition buffers, then the captured step is replayed over them), module B the
    same transitions as ordinary host-transformed fp32 batches.  The first steps warm up and capture (A captures once more
    at step 2: B's first allocation moved the allocation epoch), steps 3 and 4 are pure replays on both: the logged scalars
    of every step are equal, and so are the parameters at the end."""
    rp, ix = _replay()
    frames = _dataset()[0]
    gen = torch.Generator(device=DEV).manual_seed(21)
    ma, mb = _module("bf16"), _module("bf16")
    ma.enable_graph(); mb.enable_graph()
    seen, logs = [], []
    for _ in range(4):
        b = rp.batch(ix.draw_device(B, DEV, gen), fused=True)
        ordinary = _host_fp32(frames, b["replay"]["ids"], b, ["rgb_static"], ["rgb_static"])
        seen.append(b["replay"]["ids"].clone())
        ma.logged, mb.logged = {}, {}
        a = _step(ma, b)
        assert a == _step(mb, ordinary), a
        logs.append(a)
    assert len(ma._graphs) == 1 and len(mb._graphs) == 1  # one capture each, replayed by the later steps
    assert all(not torch.equal(seen[i], seen[i + 1]) for i in range(3)) and all(logs[i] != logs[i + 1] for i in range(3))
    sa, sb = ma.state_dict(), mb.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    rp.check()


def test_batches_survive_a_trainer_that_fetches_ahead():
    """The replay's buffers are a ring: a batch drawn now is intact after the next ones have been drawn (a trainer that looks
    one batch ahead), and comes round again only after `slots` draws."""
    from tacorl_amd.data.replay import HbmTransitionReplay

    frames, acts, nn = _dataset()
    ix = _all_strategies(EP, N, nn)
    rp = HbmTransitionReplay({"rgb_static": frames["rgb_static"]}, acts, ix, device=DEV, batch_size=B, slots=3)
    gen = torch.Generator(device=DEV).manual_seed(51)
    first = rp.batch(ix.draw_device(B, DEV, gen), fused=False)
    keep = _clone(first)
    later = [rp.batch(ix.draw_device(B, DEV, gen), fused=False) for _ in range(2)]
    torch.cuda.synchronize()
    same = lambda x, y: all(torch.equal(x[k], y[k]) for k in ("actions", "rewards", "terminals")) and torch.equal(  # noqa: E731
        x["observations"]["goal"]["rgb_static"], y["observations"]["goal"]["rgb_static"])
    assert same(first, keep) and not same(later[0], keep) and not same(later[1], keep)
    assert first["actions"].data_ptr() not in {b["actions"].data_ptr() for b in later}
    again = rp.batch(ix.draw_device(B, DEV, gen), fused=False)  # the fourth draw of a ring of three reuses the first slot
    assert again["actions"].data_ptr() == first["actions"].data_ptr()
    rp.check()


def test_validation_step_from_a_loader_leaves_the_parameters():
    from tacorl_amd.data.augment import AugmentSpec
    from tacorl_amd.data.replay import TransitionLoader

    rp, _ = _replay()
    specs = {"rgb_static": AugmentSpec(pad=4)}
    gen = torch.Generator(device=DEV).manual_seed(31)
    val = list(_clone(b) for b in TransitionLoader(rp, B, 2, aug_specs=specs, generator=gen, train=False))
    assert len(val) == 2 and all("aug" not in b and b["replay"]["B"] == B for b in val)
    assert "aug" in next(iter(TransitionLoader(rp, B, 1, aug_specs=specs, generator=gen)))
    m = _module("bf16")
    before = {k: v.clone() for k, v in m.state_dict().items()}
    out = _step(m, val[0], "validation_step")
    assert "validation/q1_loss" in out
    after = m.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    _step(m, val[1])  # ... and a training step does move them
    assert not all(torch.equal(before[k], v) for k, v in m.state_dict().items())


def test_trainer_fit_over_the_transition_loader():
    from tacorl_amd import lightning as L
    from tacorl_amd.data.augment import AugmentSpec
    from tacorl_amd.data.replay import TransitionLoader

    rp, _ = _replay()
    gen = torch.Generator(device=DEV).manual_seed(41)
    specs = {"rgb_static": AugmentSpec(pad=4)}
    train = TransitionLoader(rp, B, 3, aug_specs=specs, generator=gen)
    val = TransitionLoader(rp, B, 1, aug_specs=specs, generator=gen, train=False)
    assert len(train) == 3
    m = _module("bf16")
    m.enable_graph()
    tr = L.MiniTrainer(max_epochs=1, log_every_n_steps=1)
    tr.fit(m, train_dataloaders=train, val_dataloaders=val)
    torch.cuda.synchronize()
    assert tr.global_step == 3 and m._graphs  # the steps ran as captured graphs
    assert np.isfinite(m.logged["train/q1_loss"]) and np.isfinite(m.logged["validation/q1_loss"])
    assert np.isfinite(tr.logged_metrics["train/q1_loss"])
    rp.check()
