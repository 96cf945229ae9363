"""The dataset key `frame_dir` without a GPU (tacorl_amd/data/frame_dir.py): the compaction, the tables, the refusals, the
cache, the ring's bound, PlayDataModule on device="cpu" against what the unmodified reference PlayDataset returned on the same
directory (tests/golden/frame_dir.npz, tools/gen_frame_dir_golden.py) - and the arithmetic facts that the GPU tests of
tacorl_resize_frames_u8 rest on (tests/frame_ref.py)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import frame_ref as R

G, CFG = R.golden()
CAMS = CFG["cameras"]


@pytest.fixture(scope="module")
def gdir(tmp_path_factory):
    """The golden directory with ep_start_end_ids.npy, and its arrays by step: built once, never written."""
    root = tmp_path_factory.mktemp("frame_dir_npy")
    data, _ = R.build_golden_dir(root, "npy")
    return str(root), data


def _dm(root, **over):
    from tacorl_amd.data.play_replay import PlayDataModule

    kw = dict(batch_size=4, val_percentage=0.0, device="cpu")
    kw.update({k: over.pop(k) for k in list(over) if k in ("batch_size", "val_percentage", "device", "transform_manager", "fused")})
    return PlayDataModule(R.dataset_cfg(CFG, frame_dir=root, **over), **kw)


def _items(dm):
    """What the datamodule's replay yields for the golden's draws, on the host: window rows, goal row, padded actions."""
    from tacorl_amd.data.replay import pad_actions

    d = R.golden_draws(G)
    s = dm.index.sample(d["idx"], d)
    acts = dm.train_replay.tables["actions"].numpy()
    return s, pad_actions(acts, s["frames"], s["padded"])


# ------------------------------------------------------------------------------------------------------- the directory
def test_compaction_round_trips(gdir):
    from tacorl_amd.data.frame_dir import FrameDirectory

    root, data = gdir
    fd = FrameDirectory(root, "train", CAMS)
    ep = np.array(CFG["train_ep"])
    assert fd.n == 60 and fd.first_step == 1000 and (fd.prefix, fd.n_digits) == ("episode_", 7)
    assert np.array_equal(fd.ep, [[0, 29], [30, 59]]) and np.array_equal(fd.ep_steps, ep)
    assert np.array_equal(fd.rows(fd.step_of_row), np.arange(60)) and np.array_equal(fd.step_of_row[fd.rows(ep)], ep)
    assert np.array_equal(fd.step_of_row, np.r_[1000:1030, 1040:1070])
    assert (fd.row_of_step[30:40] == -1).all() and len(fd.row_of_step) == 70  # the gap holds no row
    for bad in (999, 1035, 1070):
        with pytest.raises(ValueError, match=str(bad)):
            fd.rows([1000, bad])
    assert fd.file_of(1005).endswith("episode_0001005.npz") and fd.stats["files_opened"] == 0
    with pytest.raises(FileNotFoundError, match="episode_000001000.npz"):  # n_digits given: the name is built with it
        FrameDirectory(root, "train", CAMS, n_digits=9)


def test_tables_name_the_frames_the_golden_names(gdir):
    """The remapped episode and neighbour tables: every window row and goal row of the golden's draws is the step the
    reference loaded, and the loaded frames at those rows are the reference's frames."""
    root, data = gdir
    dm = _dm(root)
    dm.setup()
    s, _ = _items(dm)
    sp = dm.splits["train"]
    assert np.array_equal(sp.step_of_row[s["frames"]], G["steps"]) and np.array_equal(sp.step_of_row[s["goal"]], G["goal_step"])
    assert np.array_equal(s["disp"], G["disp"]) and np.array_equal(s["window_size"], G["window_size"]) and len(dm.index) == int(G["len"])
    nn = {int(k): v for k, v in json.loads(str(G["nn"])).items()}
    tab = dm.index.nn_table.to_dict()
    assert {int(sp.step_of_row[k]): sp.step_of_row[v].tolist() for k, v in tab.items()} == nn


@pytest.mark.parametrize("table", ["npy", "split", "both"])
def test_datamodule_yields_the_goldens_frames_and_actions(table, gdir, tmp_path):
    """PlayDataModule(frame_dir=...) on device="cpu": the golden's frames (both cameras, window and goal) and padded actions
    bit for bit, with either table form."""
    root = gdir[0]
    if table != "npy":
        root = str(tmp_path / table)
        R.build_golden_dir(root, table)
    dm = _dm(root)
    dm.setup()
    s, acts = _items(dm)
    assert acts.dtype == np.float32 and np.array_equal(acts, G["actions"])
    for c in CAMS:
        fr = dm.train_replay.frames[c].numpy()
        assert fr.shape == (60, 8, 8, 3) and fr.dtype == np.uint8
        assert np.array_equal(fr[s["frames"]], G[f"frames/{c}"]) and np.array_equal(fr[s["goal"]], G[f"goal/{c}"])


def test_root_with_both_splits_and_single_directory(tmp_path, gdir):
    """A root holding training/ and validation/: each replay has its own arrays.  A single directory with split.json: both
    tables over one shared array, whose rows are the steps either table covers."""
    root = tmp_path / "root"
    tr, _ = R.build_golden_dir(root / "training", "npy")
    from tools.make_frame_dir import make_frame_dir, stacked

    va = make_frame_dir(str(root / "validation"), CFG["val_ep"], None, (8, 8), seed=3, table="npy")
    dm = _dm(str(root), val_percentage=1.0, include_goal=False)
    dm.setup()
    a, b = dm.train_replay, dm.val_replay
    assert a.frames["rgb_static"] is not b.frames["rgb_static"] and b.frames["rgb_static"].shape[0] == 20
    assert np.array_equal(b.frames["rgb_gripper"].numpy(), stacked(va, CFG["val_ep"], "rgb_gripper"))
    assert np.array_equal(a.frames["rgb_static"].numpy(), stacked(tr, CFG["train_ep"], "rgb_static"))
    assert np.array_equal(b.index.ep, [[0, 19]]) and np.array_equal(b.tables["actions"].numpy(), stacked(va, CFG["val_ep"], "rel_actions_world"))
    one = tmp_path / "one"
    data, _ = R.build_golden_dir(one, "split")
    dm = _dm(str(one), val_percentage=1.0, include_goal=False, action_type="rel_actions_gripper")
    dm.setup()
    a, b = dm.train_replay, dm.val_replay
    assert a.frames["rgb_static"] is b.frames["rgb_static"] and a.frames["rgb_static"].shape[0] == 80
    assert np.array_equal(a.index.ep, [[0, 29], [30, 59]]) and np.array_equal(b.index.ep, [[60, 79]])
    assert np.array_equal(a.tables["actions"].numpy(), stacked(data, CFG["train_ep"] + CFG["val_ep"], "rel_actions_gripper"))
    assert dm.val_dataloader() is not None
    with pytest.raises(KeyError, match="ep_start_end_ids_val"):  # ep_start_end_ids.npy alone holds no validation table
        _dm(gdir[0], val_percentage=1.0, include_goal=False).setup()


# --------------------------------------------------------------------------------------------------------- the refusals
class _NoUpload:
    """Counts the chunk copies towards the frames' device (frame_dir._copy_chunk: every frame byte that is uploaded passes
    there): nothing may be copied before a refusal."""

    def __enter__(self):
        from tacorl_amd.data import frame_dir as F

        self.F, self.orig, self.calls = F, F._copy_chunk, 0

        def counted(*a, **k):
            self.calls += 1
            return self.orig(*a, **k)

        F._copy_chunk = counted
        return self

    def __exit__(self, *a):
        self.F._copy_chunk = self.orig


def test_refusals_come_before_any_upload(tmp_path):
    from tacorl_amd.data.play_replay import PlayDataModule

    def fresh(name):
        R.build_golden_dir(tmp_path / name, "npy")
        return str(tmp_path / name)

    with _NoUpload() as up:
        d = fresh("missing_file")
        os.remove(os.path.join(d, "episode_0001047.npz"))
        with pytest.raises(FileNotFoundError, match="episode_0001047.npz"):
            _dm(d).setup()
        d = fresh("missing_key")
        with pytest.raises(KeyError, match="episode_0001000.npz.*rel_actions_none"):
            _dm(d, action_type="rel_actions_none").setup()
        with pytest.raises(KeyError, match="episode_0001000.npz.*rgb_tactile"):
            _dm(d, modalities=["rgb_static", "rgb_tactile", "rel_actions_world"]).setup()
        ds = R.dataset_cfg(CFG, frame_dir=d)
        for other in ({"path": "play.npz"}, {"arrays": {}}):
            with pytest.raises(ValueError, match="exactly one"):
                PlayDataModule(dict(ds, **other), device="cpu")
        with pytest.raises(ValueError, match="path"):
            PlayDataModule({k: v for k, v in ds.items() if k != "frame_dir"}, device="cpu")  # none: the wording that was
        with pytest.raises(ValueError, match="store_size"):
            PlayDataModule(dict(R.dataset_cfg(CFG), arrays={"frames": {}}, store_size=[8, 8]), device="cpu")
        with pytest.raises(NotImplementedError, match="GPU"):  # the resize is a HIP kernel: no eager stand-in on the host
            _dm(d, store_size=[4, 4]).setup()
        for k, v in (("cache_dir", "c"), ("workers", 2), ("chunk_frames", 8), ("ring", 2)):  # keys of the frame_dir source
            with pytest.raises(ValueError, match=k):
                PlayDataModule(dict(R.dataset_cfg(CFG), arrays={"frames": {}}, **{k: v}), device="cpu")
        # a frame whose shape differs from the first frame's - in the sixth chunk of eight - is refused with its name before
        # the first chunk is copied: every file's array headers are read when the load is planned
        d = fresh("shape_change")
        z = dict(np.load(os.path.join(d, "episode_0001050.npz")))
        z["rgb_gripper"] = np.zeros((4, 4, 3), np.uint8)
        np.savez_compressed(os.path.join(d, "episode_0001050.npz"), **z)
        with pytest.raises(ValueError, match="episode_0001050.npz.*rgb_gripper"):
            _dm(d, chunk_frames=8).setup()
        z.pop("rel_actions_world")  # ... and a key that a later frame lacks
        z["rgb_gripper"] = np.zeros((8, 8, 3), np.uint8)
        np.savez_compressed(os.path.join(d, "episode_0001050.npz"), **z)
        with pytest.raises(KeyError, match="episode_0001050.npz.*rel_actions_world"):
            _dm(d, chunk_frames=8).setup()
        # validation batches carry no resize: known from the planned sizes, refused before the load
        tm = {"transforms": {"train": {"rgb_static": [{"_target_": "torchvision.transforms.Resize", "size": 16}]}}}
        R.build_golden_dir(tmp_path / "split", "split")
        with pytest.raises(NotImplementedError, match="store the frames"):
            _dm(str(tmp_path / "split"), transform_manager=tm, val_percentage=1.0).setup()
        assert up.calls == 0
    with _NoUpload() as up:  # (the counter counts: a load that goes through copies 60 frames in 8 chunks per camera)
        _dm(fresh("fine"), chunk_frames=8).setup()
        assert up.calls == 8 * len(CAMS)


# ------------------------------------------------------------------------------------------------- the cache, the ring
def test_second_start_reads_the_cache_and_opens_no_frame_file(tmp_path):
    d = str(tmp_path / "data")
    R.build_golden_dir(d, "npy")
    cache = str(tmp_path / "cache")
    first = _dm(d, cache_dir=cache, chunk_frames=16)
    first.setup()
    st = first.load_stats["train"]
    assert st["files_opened"] == 61 and st["headers_checked"] == 60 and not st["from_cache"]  # the first frame: probed, decoded
    (key,) = os.listdir(cache)
    assert {"frames_rgb_static.npy", "frames_rgb_gripper.npy", "actions.npy", "robot_obs.npy", "ep.npy", "step_of_row.npy",
            "row_of_step.npy", "done"} <= set(os.listdir(os.path.join(cache, key)))
    for f in os.listdir(d):  # the frame files become unreadable: no permission, and nothing np.load could parse
        if f.endswith(".npz"):
            with open(os.path.join(d, f), "wb") as h:
                h.write(b"unreadable")
            os.chmod(os.path.join(d, f), 0)
    second = _dm(d, cache_dir=cache, chunk_frames=16)
    second.setup()
    st = second.load_stats["train"]
    assert st["files_opened"] == 0 and st["headers_checked"] == 0 and st["from_cache"]
    for c in CAMS:
        assert torch.equal(second.train_replay.frames[c], first.train_replay.frames[c])
    assert torch.equal(second.train_replay.tables["actions"], first.train_replay.tables["actions"])
    assert np.array_equal(second.index.ep, first.index.ep) and np.array_equal(second.index.episode_lookup, first.index.episode_lookup)
    assert np.array_equal(second.splits["train"].step_of_row, first.splits["train"].step_of_row)
    s, acts = _items(second)
    assert np.array_equal(acts, G["actions"]) and np.array_equal(second.train_replay.frames["rgb_static"].numpy()[s["frames"]], G["frames/rgb_static"])
    with pytest.raises(OSError, match="episode_0001000.npz"):  # another key is another cache: it has to read the files
        _dm(d, cache_dir=cache, action_type="rel_actions_gripper").setup()
    assert os.listdir(cache) == [key]


@pytest.mark.parametrize("workers", [1, 4, 64])
def test_the_loader_holds_no_more_than_the_ring(workers, gdir):
    """The reader's own counters: host chunk buffers are allocated once, ring x cameras of them, chunk_frames x frame_bytes
    each - 60 frames pass through 3 x 8 slots - and the pool is never wider than 16."""
    from tacorl_amd.data import frame_dir as F

    st, seen = {}, []
    orig = F.ThreadPoolExecutor
    F.ThreadPoolExecutor = lambda max_workers: (seen.append(max_workers), orig(max_workers=max_workers))[1]
    try:
        sp = F.load_split(gdir[0], "train", CAMS, "rel_actions_world", "cpu", stats=st, workers=workers, chunk_frames=8, ring=3)
    finally:
        F.ThreadPoolExecutor = orig
    assert seen == [min(workers, 16)] * 2 and st["files_opened"] == 61  # the header pass and the decode
    assert st["host_buffers"] == 3 * len(CAMS) and st["host_bytes"] == 3 * 8 * (8 * 8 * 3) * len(CAMS)
    assert st["host_bytes"] < sp.frames["rgb_static"].numel()  # less than one camera of the dataset
    assert np.array_equal(sp.frames["rgb_gripper"].numpy(), np.stack([gdir[1][s]["rgb_gripper"] for s in sp.step_of_row]))


# ---------------------------------------------------------------------- what the GPU tests of the resize kernel rest on
@pytest.mark.parametrize("src,dst", R.EXACT_SHAPES)
@pytest.mark.parametrize("kind", ["random", "all255", "checker"])
def test_exact_shapes_are_exact_in_fp32(src, dst, kind):
    """On the shapes the kernel must match bit for bit, the fp32 evaluation of the definition rounds as the fp64 one does:
    it is exact for the dyadic ratios, ties included, and for 5/3 no value lies near a tie (tests/frame_ref.py says why)."""
    f = R.kernel_frames(5, src, 11, kind)
    want = R.resize_u8(f, *dst, np.float64)
    assert np.array_equal(R.resize_u8(f, *dst, np.float32), want)
    if src == dst:
        assert np.array_equal(want, f)
    dist = R.tie_distance(f, *dst)
    if src == (40, 40):
        assert (dist > 0.05).all()  # ninths: no tie, none near one
    else:
        assert np.array_equal(R.values(f, *dst, np.float32), R.values(f, *dst, np.float64))  # dyadic: fp32 is exact
    if kind == "all255":
        assert (want == 255).all()
    if src == (25, 25) and kind == "random":
        assert (dist == 0).any()  # ties are there to be rounded to even


@pytest.mark.parametrize("src,dst", R.GENERAL_SHAPES)
def test_general_shapes_stay_inside_the_fp32_bound(src, dst):
    """The frames of the GPU test (seed 21): the fp32 evaluation differs from fp64 by at most 1, only where fp64 lies closer
    to a rounding boundary than fp32_bound, and on at most 0.5 % of the outputs."""
    f = R.kernel_frames(65, src, 21)
    a, b = R.resize_u8(f, *dst, np.float32).astype(int), R.resize_u8(f, *dst, np.float64).astype(int)
    diff = a != b
    print("differing outputs:", int(diff.sum()), "of", diff.size, "bound", R.fp32_bound(*src))
    assert np.abs(a - b).max() <= 1 and (R.tie_distance(f, *dst)[diff] < R.fp32_bound(*src)).all()
    assert diff.mean() <= R.MAX_DIFF_SHARE
    assert np.abs(R.values(f, *dst, np.float32) - R.values(f, *dst, np.float64)).max() < R.fp32_bound(*src)
    assert R.fp32_bound(*src) < 0.01


def test_ril_datamodule_reads_the_directory(gdir):
    from tacorl_amd.data.relay_replay import RILDataModule

    dm = RILDataModule({"max_low_level_window": 4, "max_high_level_window": 8, "modalities": CAMS + ["rel_actions_world"],
                        "action_type": "rel_actions_gripper", "real_world": True, "frame_dir": gdir[0]}, batch_size=4, val_percentage=0.0, device="cpu")
    dm.setup()
    want = np.stack([gdir[1][s]["rel_actions_gripper"] for s in dm.splits["train"].step_of_row])
    assert np.array_equal(dm.train_replay.tables["actions"].numpy(), want) and np.array_equal(dm.index.ep, [[0, 29], [30, 59]])
    assert dm.train_replay.frames["rgb_gripper"].shape == (60, 8, 8, 3)
    with pytest.raises(ValueError, match="exactly one"):
        RILDataModule({"frame_dir": gdir[0], "arrays": {}}, device="cpu")


def test_the_references_neighbour_file_is_found_where_the_reference_keeps_it(tmp_path):
    """The reference's JSON sits at nn_steps_from_step_path - beside training/ and validation/ - and is keyed by step number:
    it is read from there (config key, a path given outright, or the root itself), remapped to rows, and neither robot_obs nor
    a second file appears."""
    from tacorl_amd.data.frame_dir import neighbour_file

    root = tmp_path / "root"
    R.build_golden_dir(root / "training", "npy", with_nn=False)
    nn = {int(k): v for k, v in json.loads(str(G["nn"])).items()}
    for name, where in (("cfg", tmp_path / "elsewhere.json"), ("given", tmp_path / "given.json"), ("root", root / "nn_steps_from_step.json")):
        with open(where, "w") as f:
            json.dump({"train": json.loads(str(G["nn"]))}, f)
        over = {"cfg": {"nn_steps_from_step_path": str(where)}, "given": {"nn_steps_from_step": str(where)}, "root": {}}[name]
        dm = _dm(str(root), **over)
        dm.setup()
        sp = dm.splits["train"]
        assert sp.robot_obs is None and not os.path.exists(root / "training" / "nn_steps_from_step.json")
        assert {int(sp.step_of_row[k]): sp.step_of_row[v].tolist() for k, v in dm.index.nn_table.to_dict().items()} == nn, name
        if name != "root":
            os.remove(where)
    # nothing holds the validation table: it would be built into the configured file where its directory exists
    assert neighbour_file(str(root), str(root / "validation"), "validation", (None, str(tmp_path / "new.json"))) == (str(tmp_path / "new.json"), False)
    assert neighbour_file(str(root), str(root / "validation"), "validation", ("~/no/such/dir/nn.json",)) == \
        (str(root / "validation" / "nn_steps_from_step.json"), False)
    # a table given outright is in rows
    dm = _dm(str(root), nn_steps_from_step={3: [40, 59]})
    dm.setup()
    assert dm.index.nn_table is None and dm.index.nn[3].tolist() == [40, 59]
