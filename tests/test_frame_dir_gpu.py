"""tacorl_resize_frames_u8 (csrc/frame_ops.hip) against its fp64 restatement (tests/frame_ref.py), and the dataset key
`frame_dir` on the GPU: the golden directory through PlayDataModule's fused and dense samplers against what the unmodified
reference PlayDataset returned (tests/golden/frame_dir.npz), `store_size`, the entry point's refusals, one PlayLMP step."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import frame_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G, CFG = R.golden()
CAMS = CFG["cameras"]
_REF = {}


def _case(src, dst, seed):
    """65 random frames of a shape and their fp64 result: computed once, never written."""
    if (src, dst, seed) not in _REF:
        f = R.kernel_frames(65, src, seed)
        _REF[src, dst, seed] = (f, R.resize_u8(f, *dst, np.float64))
    return _REF[src, dst, seed]


def _resize(frames, dst, gap=0):
    """The kernel on host frames (n,Hs,Ws,3); gap > 0: the source frames lie frame_bytes + gap apart in a flat buffer whose
    gaps hold 0xFF, and the result goes into the middle of a sentinel-filled buffer that must stay untouched around it
    (frames of 9 x 7 are 189 bytes: every frame but the first then starts off a 16-byte boundary)."""
    from tacorl_amd import ops

    n, Hs, Ws = frames.shape[:3]
    fb = Hs * Ws * 3
    flat = np.full((n, fb + gap), 255, np.uint8)
    flat[:, :fb] = frames.reshape(n, fb)
    src = torch.from_numpy(flat.reshape(-1)).to(DEV)
    nb = n * dst[0] * dst[1] * 3
    guard = torch.full((64 + nb + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    out = guard[64:64 + nb].view(n, dst[0], dst[1], 3)
    ops.resize_frames_u8(src, out, src_pitch=(fb + gap, Hs, Ws))
    torch.cuda.synchronize()
    assert (guard[:64] == 0xA5).all() and (guard[64 + nb:] == 0xA5).all()
    return out.cpu().numpy()


@pytest.mark.parametrize("gap", [0, 37])
@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("src,dst", R.EXACT_SHAPES)
def test_kernel_equals_fp64_bit_for_bit_on_exact_ratios(src, dst, n, gap):
    f, want = _case(src, dst, 11)
    assert np.array_equal(_resize(f[:n], dst, gap), want[:n])
    for kind in ("all255", "checker"):
        e = R.kernel_frames(2, src, 0, kind)
        assert np.array_equal(_resize(e, dst, gap), R.resize_u8(e, *dst, np.float64)), kind


@pytest.mark.parametrize("gap", [0, 37])
@pytest.mark.parametrize("src,dst", R.GENERAL_SHAPES)
def test_kernel_on_a_general_ratio_stays_inside_the_fp32_bound(src, dst, gap):
    """Within 1 of fp64 everywhere; different only where fp64 lies closer to a rounding boundary than the a-priori bound of
    tests/frame_ref.py; on at most 0.5 % of the outputs (tests/test_frame_dir_cpu.py: the fp32 evaluation of these frames
    stays inside that share)."""
    f, want = _case(src, dst, 21)
    got = _resize(f, dst, gap).astype(int)
    diff = got != want.astype(int)
    print("differing outputs:", int(diff.sum()), "of", diff.size)
    assert np.abs(got - want.astype(int)).max() <= 1
    assert (R.tie_distance(f, *dst)[diff] < R.fp32_bound(*src)).all()
    assert diff.mean() <= R.MAX_DIFF_SHARE
    assert np.array_equal(got, R.resize_u8(f, *dst, np.float32))  # the same arithmetic in the same order


def test_entry_point_refuses_bad_arguments_and_leaves_the_destination_untouched():
    from tacorl_amd import _lib

    fn = getattr(_lib.lib(), "tacorl_resize_frames_u8")
    EINVAL = -22
    src = torch.zeros(4 * 40 * 40 * 3 + 64, dtype=torch.uint8, device=DEV)
    dst = torch.full((4 * 24 * 24 * 3 + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    s, d, fs, fd = src.data_ptr(), dst.data_ptr(), 40 * 40 * 3, 24 * 24 * 3
    ok = dict(src=s, sp=fs, dst=d, dp=fd, n=4, sh=40, sw=40, h=24, w=24)
    bad = [dict(src=None), dict(dst=None), dict(src=s + 8), dict(dst=d + 4), dict(n=0), dict(n=-1), dict(sh=0), dict(sw=-3), dict(h=0),
           dict(w=0), dict(sp=fs - 1), dict(dp=fd - 1), dict(sw=40000, sp=40 * 40000 * 3)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for over in bad:
        a = dict(ok, **over)
        rc = fn(a["src"], a["sp"], a["dst"], a["dp"], a["n"], a["sh"], a["sw"], a["h"], a["w"], st)
        assert rc == EINVAL, (over, rc)
    torch.cuda.synchronize()
    assert (dst == 0x5A).all()
    assert fn(s, fs, d, fd, 4, 40, 40, 24, 24, st) == 0
    torch.cuda.synchronize()
    assert (dst[: 4 * fd] == 0).all() and (dst[4 * fd:] == 0x5A).all()


# ------------------------------------------------------------------------------------------------------ the datamodule
@pytest.fixture(scope="module")
def gdir(tmp_path_factory):
    root = tmp_path_factory.mktemp("frame_dir_gpu")
    R.build_golden_dir(root, "npy")
    return str(root)


def _dm(root, **over):
    from tacorl_amd.data.play_replay import PlayDataModule

    kw = dict(batch_size=4, val_percentage=0.0, device=DEV)
    kw.update({k: over.pop(k) for k in list(over) if k in ("batch_size", "val_percentage", "transform_manager", "fused", "generator")})
    return PlayDataModule(R.dataset_cfg(CFG, frame_dir=root, **over), **kw)


@pytest.mark.parametrize("fused", [True, False])
def test_datamodule_yields_the_goldens_frames_and_actions(fused, gdir):
    """The golden's draws through the sampler kernel, out of a replay loaded from the directory (chunks of 16 frames through
    a ring of 2): the frames of both cameras (window and goal) and the padded actions, bit for bit."""
    dm = _dm(gdir, fused=fused, chunk_frames=16, ring=2, workers=4)
    dm.setup()
    rp = dm.train_replay
    b = rp.batch(R.golden_draws(G), fused=fused)
    torch.cuda.synchronize()
    B, T = len(G["idx"]), CFG["max_ws"]
    assert np.array_equal(b["actions"].cpu().numpy(), G["actions"]) and np.array_equal(b["disp"].cpu().numpy(), G["disp"])
    assert np.array_equal(b["window_size"].cpu().numpy(), G["window_size"])
    for c in CAMS:
        if fused:
            ids = b["replay"]["ids"]
            states, goal = rp.frames[c][ids[: B * T]].view(B, T, 8, 8, 3), rp.frames[c][ids[B * T:]]
        else:
            states, goal = b["states"][c], b["goal"][c]
        assert np.array_equal(states.cpu().numpy(), G[f"frames/{c}"]) and np.array_equal(goal.cpu().numpy(), G[f"goal/{c}"]), c
    rp.check()
    st = dm.load_stats["train"]
    assert st["host_buffers"] == 2 * len(CAMS) and st["host_bytes"] == 2 * 16 * 192 * len(CAMS) and st["files_opened"] == 61


RL = [{"_target_": "torchvision.transforms.Resize", "size": [8, 8]}, {"_target_": "tacorl.utils.transforms.RandomShiftsAug", "pad": 2},
      {"_target_": "tacorl.utils.transforms.ScaleImageTensor"},
      {"_target_": "tacorl.utils.transforms.ColorTransform", "contrast": 0.1, "brightness": 0.2, "hue": 0.02},
      {"_target_": "torchvision.transforms.Normalize", "mean": [0.5], "std": [0.5]}]
TM = {"transforms": {"train": {c: RL for c in CAMS}, "validation": {c: [RL[0], RL[2], RL[4]] for c in CAMS}}}


def test_store_size_resizes_the_chunks_and_opens_the_validation_loader(tmp_path):
    from tacorl_amd import ops
    from tools.make_frame_dir import stacked

    data, _ = R.build_golden_dir(tmp_path / "d12", "split", hw=(12, 12))
    eps = CFG["train_ep"] + CFG["val_ep"]
    # without store_size the refusal of the parent stands: nothing stores the frames at 8 x 8
    with pytest.raises(NotImplementedError, match="store the frames"):
        _dm(str(tmp_path / "d12"), transform_manager=TM, val_percentage=1.0).setup()
    dm = _dm(str(tmp_path / "d12"), transform_manager=TM, val_percentage=1.0, store_size=[8, 8], chunk_frames=32, fused=True,
             generator=torch.Generator(device=DEV).manual_seed(9))
    dm.setup()
    rp = dm.train_replay
    want = {}
    for c in CAMS:
        src = torch.from_numpy(stacked(data, eps, c)).to(DEV)
        want[c] = ops.resize_frames_u8(src, torch.empty(80, 8, 8, 3, dtype=torch.uint8, device=DEV))
        assert rp.frames[c].shape == (80, 8, 8, 3) and torch.equal(rp.frames[c], want[c]), c
        assert np.array_equal(want[c].cpu().numpy(), R.resize_u8(stacked(data, eps, c), 8, 8))  # 12 -> 8: ratio 3/2, exact
    vl, tl = dm.val_dataloader(), dm.train_dataloader()
    assert vl is not None and len(vl) >= 1 and "aug" not in next(iter(vl))
    assert all(sp.resize is None for sp in tl.aug_specs.values())  # the Resize stage is no stage
    b = next(iter(tl))
    B, T = 4, CFG["max_ws"]
    ids, aug = b["replay"]["ids"], b["aug"]
    assert not aug["resize"] and b["replay"]["frames"]["rgb_static"] is rp.frames["rgb_static"]
    for c in CAMS:  # the existing pack over the batch's frames = the same pack over the stored frames worked out above
        outs = []
        for frames in (b["replay"]["frames"][c], want[c]):
            dst = torch.full((B * T, 8, 8, 3), float("nan"), device=DEV)
            sh, ji = aug["states"][c]["shift"].contiguous(), aug["states"][c]["jitter"].contiguous()
            ops.pack_images_u8_resize_aug_batch([(frames.data_ptr(), 192, dst.data_ptr(), B * T, ids.data_ptr(), 1, sh, ji)],
                                                0, (8, 8), 8, 8, aug["pad"][c])
            outs.append(dst)
        torch.cuda.synchronize()
        assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]), c
    rp.check()


def test_one_playlmp_step_fed_from_a_frame_directory(tmp_path):
    from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP
    from tests import cfg_util as K
    from tools.make_frame_dir import make_frame_dir

    make_frame_dir(str(tmp_path / "training"), [[500, 519], [530, 549]], None, (84, 84), seed=1, table="npy")
    from tacorl_amd.data.play_replay import PlayDataModule

    ds = {"modalities": ["rgb_static", "rel_actions_world"], "min_window_size": 8, "max_window_size": 8, "pad": True,
          "frame_dir": str(tmp_path), "action_type": "rel_actions_world"}
    dm = PlayDataModule(ds, batch_size=4, val_percentage=0.0, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    torch.manual_seed(3)
    strip = lambda c: {k: v for k, v in c.items() if k not in ("_target_", "_recursive_")}  # noqa: E731
    mod = PlayLMP(**strip(K.playlmp_cfg(device=DEV, T=8)))
    b = next(iter(dm.train_dataloader()))
    assert b["replay"]["B"] == 4 and b["replay"]["T"] == 8 and dm.train_replay.frames["rgb_static"].shape == (40, 84, 84, 3)
    mod.training_step(b, 0)
    torch.cuda.synchronize()
    assert mod.logged and all(np.isfinite(v) for v in mod.logged.values()), mod.logged
    dm.train_replay.check()


def test_neighbour_table_is_built_on_step_numbers_and_written_in_the_references_form(tmp_path):
    """No nn_steps_from_step.json in the directory: the table is built with the k-NN kernel on step numbers (the margin
    filter sees step distances, the gap between the episodes included), written keyed by step number as the reference's
    set_nn_steps_from_step writes it, and remapped to rows; a second start reads the file."""
    import json
    import os

    from tacorl_amd.data.neighbours import nn_steps_from_step_host
    from tools.make_frame_dir import stacked

    data, _ = R.build_golden_dir(tmp_path / "d", "npy", with_nn=False)
    ep = np.array(CFG["train_ep"])
    ro = np.zeros((70, 15), np.float32)
    ro[np.r_[0:30, 40:70]] = stacked(data, CFG["train_ep"], "robot_obs")
    want = {k + 1000: [v + 1000 for v in vs] for k, vs in nn_steps_from_step_host(ro, ep - 1000, num_nn=12, margin=16).items()}
    assert any(want.values()) and any(a < 1030 <= b for a, vs in want.items() for b in vs)  # lists across the gap
    dm = _dm(str(tmp_path / "d"), num_nn=12)
    dm.setup()
    sp = dm.splits["train"]
    got = {int(sp.step_of_row[k]): sp.step_of_row[v].tolist() for k, v in dm.index.nn_table.to_dict().items()}
    assert got == want
    with open(os.path.join(str(tmp_path / "d"), "nn_steps_from_step.json")) as f:
        doc = json.load(f)
    assert set(doc) == {"train"} and {int(k): v for k, v in doc["train"].items()} == want
    again = _dm(str(tmp_path / "d"), num_nn=12)
    again.setup()
    assert again.splits["train"].robot_obs is None and again.index.nn_table.to_dict() == dm.index.nn_table.to_dict()
    b = dm.train_replay.batch(R.golden_draws(G), fused=True)
    torch.cuda.synchronize()
    dm.train_replay.check()


def test_transition_replay_from_a_frame_directory(gdir):
    from tacorl_amd.data.replay import HbmTransitionReplay

    rp = HbmTransitionReplay.from_frame_dir(gdir, CAMS, device=DEV, batch_size=8,
                                            goal_strategy_prob={"geometric": 0.5, "similar_robot_obs": 0.5})
    assert np.array_equal(rp.index.ep, [[0, 29], [30, 59]]) and rp.index.n_frames == 60
    nn = {int(k): v for k, v in __import__("json").loads(str(G["nn"])).items()}
    sp = rp.split
    assert {int(sp.step_of_row[k]): sp.step_of_row[v].tolist() for k, v in rp.index.nn_table.to_dict().items()} == nn
    b = rp.batch(fused=False)
    torch.cuda.synchronize()
    rp.check()
    ids = None
    f = rp.batch(fused=True)
    torch.cuda.synchronize()
    ids = f["replay"]["ids"]
    for c in CAMS:
        assert b["observations"]["observation"][c].shape == (8, 8, 8, 3)
        assert torch.equal(rp.frames[c][ids[1]], rp.frames[c][ids[0] + 1])  # the next observation is the next row


def test_store_size_with_a_frame_size_off_the_16_byte_grid(tmp_path):
    """store_size 9 x 7 is 189 bytes a frame: chunk starts of 5 frames would hand the kernel unaligned destinations, so the
    loader rounds the chunk to a multiple of 16 frames - 80 frames go through 5 chunks, and the result is the kernel's."""
    from tacorl_amd import ops
    from tools.make_frame_dir import stacked

    data, _ = R.build_golden_dir(tmp_path / "d12", "split", hw=(12, 12))
    dm = _dm(str(tmp_path / "d12"), val_percentage=1.0, include_goal=False, store_size=[9, 7], chunk_frames=5)
    dm.setup()
    assert dm.load_stats["train"]["host_bytes"] == 3 * 16 * 12 * 12 * 3 * len(CAMS)
    for c in CAMS:
        src = torch.from_numpy(stacked(data, CFG["train_ep"] + CFG["val_ep"], c)).to(DEV)
        want = ops.resize_frames_u8(src, torch.empty(80, 9, 7, 3, dtype=torch.uint8, device=DEV))
        assert torch.equal(dm.train_replay.frames[c], want), c
