"""The resident relay replay on the GPU: the sampler kernel (`tacorl_sample_relay`) against the host RelayIndex and the
reference's recorded items bit for bit, HbmRelayReplay's two batch forms, and RelayImitationLearning steps fed by them - the
fused batch (frames read by id out of the dataset), the gathered uint8 batch and the host-transformed fp32 batch must be one
step - with augmentation tables, under graph replay and through Trainer.fit(datamodule=RILDataModule)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ril_util as U
from tests.golden_util import Golden
from tests.relay_util import ROLES, RelayGolden, extreme_draws

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = RelayGolden()
N, B = 160, 4
EP, LW, HW_ = [[0, 69], [70, 159]], 4, 12  # the replay tests' index: both ranges non-empty away from the episode ends
GEOMETRY = {"rgb_static": 84, "rgb_gripper": 64}  # the `ril` / `ril_twocam` fixtures' cameras


def _sampled(ix, actions, draws):
    """(replay, its fused batch) for the draws, with nothing but the tables resident (no camera)."""
    from tacorl_amd.data.relay_replay import HbmRelayReplay

    rp = HbmRelayReplay({}, actions, ix, device=DEV, batch_size=8)
    b = rp.batch(draws, fused=True)
    torch.cuda.synchronize()
    return rp, b


def _host_ids(s):
    return np.stack([s[r] for r in ROLES])


def _assert_equals_host(ix, actions, draws):
    s = ix.sample(None, draws)
    rp, b = _sampled(ix, actions, draws)
    n = len(s["step"])
    ids = b["replay"]["ids"].cpu().numpy()
    assert ids.shape == (4, n) and b["replay"]["B"] == n and b["replay"]["kind"] == "relay"
    assert np.array_equal(ids, _host_ids(s))
    assert np.array_equal(b["low_level_action"].cpu().numpy(), np.asarray(actions, np.float32)[s["step"]])
    assert int(rp.status.item()) == 0
    rp.check()
    return ids


@pytest.mark.parametrize("variant", list(G.variants))
def test_kernel_equals_host_sampler_and_reference_on_the_recorded_draws(variant):
    ix = G.index(variant)
    acts = G.actions[: G.n_frames(variant)]
    ids = _assert_equals_host(ix, acts, G.draws(variant))
    assert np.array_equal(ids, G.ids(variant))  # ... which are the reference dataset's items
    assert ids.shape[1] == len(ix)              # every item of the variant


@pytest.mark.parametrize("n,A", [(1, 7), (255, 7), (256, 3), (257, 7), (257, 3)])
def test_kernel_equals_host_sampler_on_fresh_draws(n, A):
    """One thread per sample in 256-thread blocks: one item, a block less one, a full block, a block and one; two action
    widths; the first draws carry the extreme uniforms 0.0 and nextafter(1, 0)."""
    acts = np.random.RandomState(n + A).uniform(-1, 1, size=(N, A)).astype(np.float32)
    for variant in ("yaml_30_260", "low1_high3", "high_below_low_8_5", "high_beyond_2_1000"):
        ix = G.index(variant)
        d = extreme_draws(ix, n, 100 + n)
        d["idx"][: min(n, 2)] = [0, len(ix) - 1][: min(n, 2)]
        _assert_equals_host(ix, acts[: G.n_frames(variant)], d)


def test_device_draws_feed_the_kernel():
    """draw_device's tensors go to the kernel as they are; the host sampler on their copies gives the same batch."""
    ix = G.index("short_4_12")
    d = ix.draw_device(1000, DEV, torch.Generator(device=DEV).manual_seed(5))
    assert all(t.is_cuda for t in d.values()) and d["idx"].dtype == torch.int64 and d["u_low"].dtype == torch.float64
    assert int(d["idx"].min()) >= 0 and int(d["idx"].max()) < len(ix)
    assert float(d["u_low"].min()) >= 0.0 and float(d["u_low"].max()) < 1.0 and float(d["u_high"].max()) < 1.0
    s = ix.sample(None, {k: v.cpu().numpy() for k, v in d.items()})
    rp, b = _sampled(ix, G.actions, d)
    ids = b["replay"]["ids"].cpu().numpy()
    assert np.array_equal(ids, _host_ids(s)) and ids.min() >= 0 and ids.max() < ix.n_frames
    rp.check()


def test_entry_point_refuses_bad_arguments_without_launching():
    from tacorl_amd import _lib
    from tacorl_amd.data.relay_replay import HbmRelayReplay

    ix = G.index("short_4_12")
    rp = HbmRelayReplay({}, G.actions, ix, device=DEV, batch_size=8)
    t, n = rp.tables, 8
    d = ix.draw_device(n, DEV, torch.Generator(device=DEV).manual_seed(0))
    ids = torch.full((4, n), -7, dtype=torch.int64, device=DEV)
    act = torch.full((n, 7), -7.0, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    off = lambda x, k: C.c_void_p(x.data_ptr() + k)  # noqa: E731

    def args(**over):
        a = dict(lookup=p(t["lookup"]), n_items=t["lookup"].numel(), es=p(t["ep_start"]), ee=p(t["ep_end"]), n_ep=t["ep_start"].numel(),
                 actions=p(t["actions"]), n_frames=t["n_frames"], idx=p(d["idx"]), u_low=p(d["u_low"]), u_high=p(d["u_high"]),
                 lw=4, hw=12, B=n, A=7, ids=p(ids), action=p(act), status=p(rp.status), stream=None)
        a.update(over)
        return list(a.values())

    fn = _lib.lib().tacorl_sample_relay
    EINVAL = -22  # TACORL_EINVAL (csrc/common.h)
    for k in ("B", "A", "n_items", "n_ep", "n_frames", "lw", "hw"):
        assert fn(*args(**{k: 0})) == EINVAL and fn(*args(**{k: -3})) == EINVAL, k
    for k in ("lookup", "es", "ee", "actions", "idx", "u_low", "u_high", "ids", "action", "status"):
        assert fn(*args(**{k: None})) == EINVAL, k
    for k, tns in (("lookup", t["lookup"]), ("es", t["ep_start"]), ("ee", t["ep_end"]), ("idx", d["idx"]), ("u_low", d["u_low"]),
                   ("u_high", d["u_high"]), ("ids", ids)):
        assert fn(*args(**{k: off(tns, 4)})) == EINVAL, k  # int64 / double tables need 8 bytes
    for k, tns in (("actions", t["actions"]), ("action", act), ("status", rp.status)):
        assert fn(*args(**{k: off(tns, 2)})) == EINVAL, k  # float / int need 4
    torch.cuda.synchronize()
    assert int(ids.min()) == -7 and int(ids.max()) == -7 and float(act.min()) == -7.0 == float(act.max())  # nothing ran
    assert fn(*args(stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))) == 0
    torch.cuda.synchronize()
    assert int(ids.min()) >= 0 and int(ids.max()) < t["n_frames"] and int(rp.status.item()) == 0


def test_items_outside_the_index_are_clamped_and_reported():
    """idx = -1 and idx = len: the kernel clamps the item before it reads the lookup table (the first statement behind the
    bounds check of sample_relay_kernel), samples items 0 and len - 1 instead, and raises the status word."""
    ix = G.index("short_4_12")
    d = ix.draw(B, np.random.default_rng(9))
    d["idx"][:2] = [-1, len(ix)]
    rp, b = _sampled(ix, G.actions, d)
    ok = dict(d, idx=np.clip(d["idx"], 0, len(ix) - 1))
    assert np.array_equal(b["replay"]["ids"].cpu().numpy(), _host_ids(ix.sample(None, ok)))
    assert int(rp.status.item()) == 1
    with pytest.raises(IndexError):
        rp.check()


# ---------------------------------------------------------------------------------------------- the replay and the step
_DATA = {}


def _dataset():
    """160 uint8 frames of the two fixture cameras (and rgb_static once more, stored at 96x96) and actions: built once,
    never written."""
    if not _DATA:
        g = torch.Generator().manual_seed(3)
        _DATA["frames"] = {c: torch.randint(0, 256, (N, hw, hw, 3), dtype=torch.uint8, generator=g).to(DEV)
                           for c, hw in list(GEOMETRY.items()) + [("static96", 96)]}
        acts = np.random.RandomState(4).uniform(-1, 1, size=(N, 7)).astype(np.float32)
        acts[:, -1] = np.where(acts[:, -1] >= 0, 1.0, -1.0)
        _DATA["actions"] = acts
    return _DATA["frames"], _DATA["actions"]


def _replay(cams=("rgb_static",), stored=None, **kw):
    from tacorl_amd.data.relay_replay import HbmRelayReplay, RelayIndex

    frames, acts = _dataset()
    ix = RelayIndex(EP, n_frames=N, max_low_level_window=LW, max_high_level_window=HW_)
    return HbmRelayReplay({c: frames[(stored or {}).get(c, c)] for c in cams}, acts, ix, device=DEV, batch_size=B, **kw), ix


def _module(name="ril", compute="f32"):
    from tacorl_amd.modules.relay_imitation_learning.relay_imitation_learning import RelayImitationLearning

    g = Golden(name)
    mod = RelayImitationLearning(device=DEV, **U.cfg_of_golden(g, compute_dtype=compute, image_dtype=compute))
    mod.load_state_dict(g.params())
    return mod


def _step(mod, batch, fn="training_step"):
    mod.logged = {}
    getattr(mod, fn)(batch, 0)
    torch.cuda.synchronize()
    out = dict(mod.logged)
    assert out and all(np.isfinite(v) for v in out.values()), out
    return out


def _clone(b):
    return {k: _clone(v) if isinstance(v, dict) else (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}


def _host_fp32(frames, ids, action, cams):
    """The reference pipeline on the host: frames[ids] -> ToTensor -> Normalize(0.5, 0.5), NCHW fp32, computed by the CPU
    (a true division by 255, as the pack kernel's) and then moved."""
    hid = ids.cpu()
    t = lambda c, k: (((frames[c].cpu()[hid[k]].permute(0, 3, 1, 2).contiguous().float() / 255.0) - 0.5) / 0.5).to(DEV)  # noqa: E731
    b = {role: {c: t(c, k) for c in cams} for k, role in enumerate(ROLES)}
    b["low_level_action"] = action.clone()
    return b


def test_gathered_batch_has_the_reference_schema():
    cams = tuple(GEOMETRY)
    rp, ix = _replay(cams)
    d = ix.draw(B, np.random.default_rng(2))
    s = ix.sample(None, d)
    b = rp.batch(d, fused=False)
    torch.cuda.synchronize()
    assert set(b) == set(ROLES) | {"low_level_action"}
    frames, acts = _dataset()
    for role in ROLES:
        assert set(b[role]) == set(cams)
        for c in cams:
            got = b[role][c]
            assert got.dtype == torch.uint8 and got.shape == (B, GEOMETRY[c], GEOMETRY[c], 3)
            assert torch.equal(got, frames[c][torch.from_numpy(s[role]).to(DEV)]), (role, c)
    assert b["low_level_action"].shape == (B, 7) and np.array_equal(b["low_level_action"].cpu().numpy(), acts[s["step"]])
    rp.check()


def test_batches_survive_a_trainer_that_fetches_ahead():
    """The replay's buffers are a ring: a batch drawn now is intact after `slots - 1` later draws, and its slot comes round
    again with the draw after those."""
    rp, ix = _replay(slots=3)
    gen = torch.Generator(device=DEV).manual_seed(51)
    first = rp.batch(ix.draw_device(B, DEV, gen), fused=False)
    keep = _clone(first)
    later = [rp.batch(ix.draw_device(B, DEV, gen), fused=False) for _ in range(2)]
    torch.cuda.synchronize()
    same = lambda x, y: torch.equal(x["low_level_action"], y["low_level_action"]) and all(  # noqa: E731
        torch.equal(x[r]["rgb_static"], y[r]["rgb_static"]) for r in ROLES)
    assert same(first, keep) and not same(later[0], keep) and not same(later[1], keep)
    assert first["low_level_action"].data_ptr() not in {b["low_level_action"].data_ptr() for b in later}
    again = rp.batch(ix.draw_device(B, DEV, gen), fused=False)  # the fourth draw of a ring of three reuses the first slot
    assert again["low_level_action"].data_ptr() == first["low_level_action"].data_ptr()
    rp.check()


@pytest.mark.parametrize("name,compute", [("ril", "f32"), ("ril_twocam", "f32"), ("ril_twocam", "bf16")])
def test_ril_steps_are_the_same_from_all_three_batch_forms(name, compute):
    """Two training steps per form.  ril_twocam: the low-level and high-level modality lists differ in order."""
    cams = sorted(Golden(name).cams)
    rp, ix = _replay(cams)
    frames = _dataset()[0]
    rng = np.random.default_rng(11)
    draws = [ix.draw(B, rng) for _ in range(2)]
    outs, x3, params = [], [], []
    for form in ("fused", "gathered", "host"):
        m = _module(name, compute)
        assert sorted(m.engine.cams) == cams and (name == "ril" or m.engine.low_cams != m.engine.high_cams)
        losses = []
        for d in draws:
            b = rp.batch(d, fused=form != "gathered")
            if form == "host":
                b = _host_fp32(frames, b["replay"]["ids"], b["low_level_action"], cams)
            losses.append(_step(m, b))
        outs.append(losses)
        x3.append({c: m.engine.X3[c].clone() for c in cams})
        params.append(m.engine.blk.param.clone())
    assert outs[0] == outs[1] == outs[2], outs
    assert outs[0][0] != outs[0][1]
    for k in (1, 2):
        assert all(torch.equal(x3[0][c], x3[k][c]) for c in cams) and torch.equal(params[0], params[k]), k
    rp.check()


@pytest.mark.parametrize("resize", [None, 84])
def test_augmented_fused_equals_gathered_equals_the_pack_op(resize):
    """The same augmentation tables through the fused and the gathered route, and role by role through the augmenting pack
    entry point on the gathered frames; once with aug["resize"]: frames stored at 96x96, images 84x84."""
    from tacorl_amd import image_ingest as ingest
    from tacorl_amd import ops
    from tacorl_amd.data.augment import AugmentSpec, draw_ril_batch_augmentation
    from tacorl_amd.encoder_stage import image_flag

    cam = "rgb_static"
    rp, ix = _replay((cam,), stored={cam: "static96"} if resize else None)
    src = 96 if resize else 84
    d = ix.draw(B, np.random.default_rng(13))
    spec = AugmentSpec(pad=4, brightness=0.3, contrast=0.3, hue=0.1, resize=(resize, resize) if resize else None)
    aug = draw_ril_batch_augmentation({cam: spec}, B, DEV, torch.Generator(device=DEV).manual_seed(14))
    assert ("resize" in aug and aug["resize"] == ({cam: (84, 84)} if resize else {}))
    x3, outs = [], []
    for fused in (True, False):
        m = _module("ril", "bf16")
        b = rp.batch(d, aug=aug, fused=fused)
        assert b["aug"] is aug
        outs.append(_step(m, b))
        assert tuple(m.engine.X3[cam].shape) == (4 * B, 84, 84, 3)
        x3.append(m.engine.X3[cam].clone())
    assert torch.equal(x3[0], x3[1]) and outs[0] == outs[1]
    gathered = rp.batch(d, fused=False)
    for k, role in enumerate(ROLES):
        t = gathered[role][cam]
        assert t.shape == (B, src, src, 3)
        ref = torch.zeros(B, 84, 84, 3, device=DEV, dtype=torch.bfloat16)
        job = ingest.PackJob(t.data_ptr(), t[0].numel(), ref.data_ptr(), B, None, 1, aug[role][cam]["shift"], aug[role][cam]["jitter"])
        ops.pack_images_u8_resize_aug_batch([job], image_flag(torch.bfloat16), (src, src), 84, 84, 4)
        torch.cuda.synchronize()
        assert torch.equal(x3[0][k * B:(k + 1) * B], ref), role
    if not resize:  # ... and the tables were applied: the plain pack of the same frames gives other images
        m = _module("ril", "bf16")
        _step(m, rp.batch(d, fused=True))
        assert not torch.equal(m.engine.X3[cam], x3[0])
    rp.check()


def test_aug_needs_uint8_frames_and_the_relay_kind():
    from tacorl_amd.data.augment import AugmentSpec, draw_ril_batch_augmentation

    rp, ix = _replay()
    frames = _dataset()[0]
    d = ix.draw(B, np.random.default_rng(15))
    m = _module("ril")
    fused = rp.batch(d, fused=True)
    host = _host_fp32(frames, fused["replay"]["ids"], fused["low_level_action"], ["rgb_static"])
    host["aug"] = draw_ril_batch_augmentation({"rgb_static": AugmentSpec(pad=4)}, B, DEV, torch.Generator(device=DEV).manual_seed(1))
    with pytest.raises(ValueError, match="uint8"):
        m.training_step(host, 0)
    other = dict(fused, replay=dict(fused["replay"], kind="transition"))
    with pytest.raises(ValueError, match="relay replay"):
        m.training_step(other, 0)
    torch.cuda.synchronize()


def test_fused_batches_under_graph_replay_equal_an_eager_twin():
    """Three consecutive fused batches with different draws: the module with enable_graph() (warm-up and capture, then
    replays over image slots the eager pack refilled) logs what its eager twin logs.  Same kernels on the same inputs; the
    bound is the one tests/test_ril_gpu.py test_graph_replay_equals_eager holds graph against eager to (1e-6 relative: fp32
    atomics may sum in another order)."""
    rp, ix = _replay()
    gen = torch.Generator(device=DEV).manual_seed(21)
    ma, mb = _module("ril", "bf16"), _module("ril", "bf16")
    ma.enable_graph()
    seen, logs = [], []
    for _ in range(3):
        b = rp.batch(ix.draw_device(B, DEV, gen), fused=True)
        seen.append(b["replay"]["ids"].clone())
        a, e = _step(ma, b), _step(mb, b)
        assert a.keys() == e.keys() and all(abs(a[k] - e[k]) <= 1e-6 * max(abs(e[k]), 1e-3) for k in e), (a, e)
        logs.append(a)
    assert ma._graphs
    assert all(not torch.equal(seen[i], seen[i + 1]) for i in range(2)) and all(logs[i] != logs[i + 1] for i in range(2))
    rp.check()


RL = {"transforms": {"train": {"rgb_static": [{"_target_": "tacorl.utils.transforms.RandomShiftsAug", "pad": 4},
                                              {"_target_": "tacorl.utils.transforms.ScaleImageTensor"},
                                              {"_target_": "tacorl.utils.transforms.ColorTransform", "contrast": 0.1, "brightness": 0.1, "hue": 0.02},
                                              {"_target_": "torchvision.transforms.Normalize", "mean": [0.5], "std": [0.5]}]},
                     "validation": {"rgb_static": [{"_target_": "tacorl.utils.transforms.ScaleImageTensor"},
                                                   {"_target_": "torchvision.transforms.Normalize", "mean": [0.5], "std": [0.5]}]}}}


@pytest.mark.parametrize("fused", [True, False])
def test_trainer_fit_over_the_datamodule(fused, tmp_path):
    from tacorl_amd import lightning as L
    from tacorl_amd.data import RILDataModule

    frames, acts = _dataset()
    path = str(tmp_path / "ril.npz")
    np.savez(path, **{"frames/rgb_static": frames["rgb_static"][:120].cpu().numpy(), "actions": acts[:120],
                      "ep_start_end_ids_train": np.array([[0, 79]]), "ep_start_end_ids_val": np.array([[80, 119]])})
    dm = RILDataModule({"max_low_level_window": LW, "max_high_level_window": HW_, "path": path}, batch_size=B, train_percentage=0.5,
                       val_percentage=0.5, transform_manager=RL, steps_per_epoch=2, val_steps=1, device=DEV, fused=fused,
                       generator=torch.Generator(device=DEV).manual_seed(41))
    train, val = list(map(_clone, dm.train_dataloader())), list(map(_clone, dm.val_dataloader()))
    assert len(train) == 2 and len(val) == 1 and all("aug" in b for b in train) and all("aug" not in b for b in val)
    assert all(("replay" in b) == fused for b in train + val)
    assert len(dm.train_replay.index) == int(76 * 0.5) and len(dm.val_replay.index) == int(36 * 0.5)
    m = _module("ril", "bf16")
    tr = L.MiniTrainer(max_epochs=2, log_every_n_steps=1)
    tr.fit(m, datamodule=dm)
    torch.cuda.synchronize()
    assert tr.global_step == 4
    for k in ("low_level_loss", "high_level_loss", "total_loss"):
        assert np.isfinite(m.logged[f"train/{k}"]) and np.isfinite(m.logged[f"validation/{k}"]), m.logged
    dm.train_replay.check()
    dm.val_replay.check()
