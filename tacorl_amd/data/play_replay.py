"""The play-window data path on the device (`experiment=tacorl`, `play_lmp_for_rl` and the real-world variants): the dataset
resident in HBM with one sampler launch per batch (HbmPlayReplay, `tacorl_sample_play_windows` - PlayIndex.sample and
pad_actions of data/replay.py as index arithmetic over resident tables), and the loader / datamodule that `Trainer.fit`
takes (PlayWindowLoader, PlayDataModule - the counterpart of the reference's datamodule/basic_data_module.py BasicDataModule
with the PlayDataset configs).  Beside data/replay.py's HbmReplay / prefetching, which sample on the host and stage every
batch through pinned memory on a feeder thread: here the trainer's own thread enqueues the draws and the sampler in front of
the step, and nothing is synchronised, copied or allocated per batch.
"""
import os

import numpy as np
import torch

from .. import ops
from .augment import draw_play_batch_augmentation
from .relay_replay import augment_specs
from .replay import PlayIndex, _is_table

DRAW_KEYS = ("idx", "window_size", "strategy", "disp", "noise_step", "u_choice", "u_random_state")


def validate_play_tables(index, n_frames):
    """The tables of a PlayIndex against a dataset of n_frames frames, once: the episode bounds lie inside [0, n_frames), the
    episodes are sorted by start and do not overlap, every item leaves room for a max-size window inside its episode
    (episode_lookup[i] + max_ws - 1 <= the end of the episode that holds it), and every neighbour key and value lies inside
    [0, n_frames).  Every id the sampler's arithmetic can then produce is a frame of the dataset - the window
    s .. s + ws - 1 <= end, a geometric goal <= end (clipped at 0), a neighbour checked one by one, a random state another
    item - which is what the unchecked device gathers behind it rely on."""
    n_frames = int(n_frames)
    ep = np.asarray(index.ep, dtype=np.int64).reshape(-1, 2)
    if len(ep) == 0:
        raise ValueError("play replay: no episodes")
    if index.min_ws < 1:
        raise ValueError(f"play replay: min_window_size {index.min_ws} < 1")
    if n_frames < index.max_ws:
        raise ValueError(f"play replay: {n_frames} frames hold no window of {index.max_ws}")
    if ep.min() < 0 or ep.max() >= n_frames:
        raise ValueError(f"play replay: episode bounds outside [0, {n_frames})")
    if (ep[:, 0] > ep[:, 1]).any() or (ep[1:, 0] <= ep[:-1, 1]).any():
        raise ValueError("play replay: episodes must be sorted by start and must not overlap")
    look = np.asarray(index.episode_lookup, dtype=np.int64)
    if len(look) == 0:
        raise ValueError("play replay: the index has no item")
    end = index.episode_end(look)  # -1 where an item lies in no episode
    if (look < 0).any() or (look + index.max_ws - 1 > end).any():
        raise ValueError("play replay: an item's max-size window leaves its episode")
    ptr, val = np.asarray(index._nn_ptr, dtype=np.int64), np.asarray(index._nn_val, dtype=np.int64)
    keys = index.nn_table.host()[2] if index.nn_table is not None else np.array(sorted(index.nn or {}), dtype=np.int64)
    if (len(keys) and (keys.min() < 0 or keys.max() >= n_frames)) or len(ptr) - 1 > n_frames:
        raise ValueError(f"play replay: nn_steps_from_step has a key outside [0, {n_frames})")
    if len(val) and (val.min() < 0 or val.max() >= n_frames):
        raise ValueError(f"play replay: nn_steps_from_step has a neighbour outside [0, {n_frames})")
    if len(ptr) < 1 or ptr[0] != 0 or (np.diff(ptr) < 0).any() or ptr[-1] > len(val):
        raise ValueError("play replay: the neighbour CSR is not a row pointer over its values")


class HbmPlayReplay:
    """The play-window batches out of a dataset resident in HBM: frames[cam] = (N,H,W,3) uint8, the (N,A) action table and
    the index tables (episode_lookup, the episode bounds, the neighbour CSR) all live on the device, and `batch()` is one
    launch of the sampler kernel (`tacorl_sample_play_windows`) on the current stream - no host synchronisation, nothing
    over PCIe, no feeder thread.  The tables are validated here, once (validate_play_tables).
    The returned tensors are views of this object's own buffers, a ring of `slots` sets (as HbmTransitionReplay's): a batch
    stays valid until `slots - 1` more have been drawn, so a trainer that fetches a batch or two ahead of the step it runs
    still trains on the batch it was given.
    include_goal=False (PlayLMP's dataset, config/datamodule/dataset/play_dataset.yaml): the batch carries no `goal` and no
    `disp`, as the reference's."""

    def __init__(self, frames, actions, index, device=None, batch_size=64, slots=6, include_goal=True):
        acts = torch.as_tensor(np.asarray(actions, dtype=np.float32) if not torch.is_tensor(actions) else actions)
        frames = {c: torch.as_tensor(v) for c, v in frames.items()}
        self.dev =torch.device(device) if device is not None else (next(iter(frames.values())).device if frames else acts.device)
        self.index, self.batch_size, self.include_goal = index, int(batch_size), bool(include_goal)
        bad = [c for c, v in frames.items() if v.dtype != torch.uint8 or v.dim() != 4]
        if bad or acts.dim() != 2:
            raise ValueError(f"frames must be uint8 (N,H,W,3) and actions (N,A): {bad or tuple(acts.shape)}")
        n_frames = min([int(v.shape[0]) for v in frames.values()] + [int(acts.shape[0])])
        validate_play_tables(index, n_frames)
        if int(slots) < 1:
            raise ValueError("slots must be >= 1")
        self.frames = {c: v.to(self.dev).contiguous() for c, v in frames.items()}
        acts = acts.to(self.dev, torch.float32).contiguous()
        i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(self.dev)  # noqa: E731
        tab = index.nn_table
        if tab is not None and tab.val.numel() and tab.device == torch.empty(0, device=self.dev).device:
            # a NeighbourTable built on this device: its tensors are the sampler's tables (ptr cut as the index keeps it)
            nn_ptr, nn_val = tab.ptr[: len(index._nn_ptr)], tab.val
        else:
            nn_ptr, nn_val = i64(index._nn_ptr), i64(index._nn_val if len(index._nn_val) else [0])
        self.tables = {"lookup": i64(index.episode_lookup), "ep_start": i64(index.ep[:, 0]), "ep_end": i64(index.ep[:, 1]),
                       "nn_ptr": nn_ptr, "nn_val": nn_val, "actions": acts, "n_nn": len(index._nn_ptr) - 1,
                       "n_frames": n_frames, "last_end": int(index.ep[:, 1].max())}
        self.A, self.T = int(acts.shape[1]), index.max_ws
        self.status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._cap, self._ring, self._k, self._u8 = 0, [{} for _ in range(int(slots))], 0, {}
        self._grow(self.batch_size)

    def _grow(self, B):
        """The batch buffers exist before the first batch and are replaced only for a larger one - under the capture lock,
        and captured graphs that could hold an old address are dropped (as HbmD4RLReplay._grow)."""
        if B <= self._cap:
            return
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=self.dev)  # noqa: E731
        with ops.capture_lock:
            for k in range(len(self._ring)):
                self._ring[k] = {"ids": z(B * self.T + B, torch.int64), "act": z(B * self.T * self.A, torch.float32),
                                 "disp": z(B, torch.int64), "window_size": z(B, torch.int64)}
            self._cap = B
            ops.note_alloc()

    def _out(self, key, shape):
        n = int(np.prod(shape))
        t = self._u8.get(key)
        if t is None or t.numel() < n:
            with ops.capture_lock:
                t = self._u8[key] = torch.empty(n, dtype=torch.uint8, device=self.dev)
                ops.note_alloc()
        return t[:n].view(shape)

    def check(self):
        """Reads the sampler's status word back (a host synchronisation: call it when you ask, not per step)."""
        if int(self.status.item()) != 0:
            raise IndexError("play replay: the sampler had to clamp a value (tables or draws outside the dataset)")

    def _draws(self, draws, batch_size=None):
        if draws is None:
            return self.index.draw_device(batch_size or self.batch_size, self.dev)
        d = {}
        for k in DRAW_KEYS:
            if k not in draws:
                raise KeyError(f"play replay: the draws have no `{k}` (PlayIndex.draw_device, or draw() plus `idx`)")
            v = draws[k]
            if not torch.is_tensor(v):  # the host form (PlayIndex.draw): a pageable copy - tests and tools, not the training path
                v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64 if k.startswith("u_") else np.int64))
            d[k] = v.to(self.dev).contiguous()
        if self.index.min_ws == self.index.max_ws:  # the window is no draw (PlayIndex.sample ignores it too)
            d["window_size"] = self.index.device_constants(int(d["idx"].numel()), self.dev)[0]
        return d

    def batch(self, draws=None, aug=None, fused=True, batch_size=None):
        """draws: PlayIndex.draw_device(...) (None: drawn here for `batch_size`), or the host form `draw(...)` with `idx`.
        The schema is HbmReplay.batch's without `ready` (there is no copy stream to wait for):
        fused=True: no frame moves here - the batch carries the dataset tensors and the id table [B*T window frames | B goal
        frames] (`batch["replay"]`), and the module's image pack reads the frames by id on their way into the encoder.
        fused=False: `states` (B,T,H,W,3) / `goal` (B,H,W,3) uint8 per camera, gathered here (tacorl_gather_frames_u8).
        Both: `actions` (B,T,A) f32, `disp`, `idx`, `window_size` (B) int64 on the device, and `aug` where given."""
        d = self._draws(draws, batch_size)
        B, T = int(d["idx"].numel()), self.T
        self._grow(B)
        self._k = slot = (self._k + 1) % len(self._ring)
        buf = self._ring[slot]
        ids, act = buf["ids"][: B * T + B], buf["act"][: B * T * self.A].view(B, T, self.A)
        disp, ws = buf["disp"][:B], buf["window_size"][:B]
        ops.sample_play_windows(self.tables, d, T, self.index.min_ws, ids, act, disp, ws, self.status,
                                goal_augmentation=self.index.goal_augmentation)
        b = {"actions": act, "idx": d["idx"], "window_size": ws}
        if self.include_goal:
            b["disp"] = disp
        if aug is not None:
            b["aug"] = aug
        if fused:
            b["replay"] = {"frames": self.frames, "ids": ids, "B": B, "T": T}
            return b
        states, goal = {}, {}
        for c, fr in self.frames.items():
            H, W = fr.shape[1:3]
            states[c] = ops.gather_frames_u8(fr, ids[: B * T], self._out((slot, "s", c), (B, T, H, W, 3)))
            if self.include_goal:
                goal[c] = ops.gather_frames_u8(fr, ids[B * T:], self._out((slot, "g", c), (B, H, W, 3)))
        b["states"] = states
        if self.include_goal:
            b["goal"] = goal
        return b


class PlayWindowLoader:
    """`steps_per_epoch` batches of `batch_size` fresh device draws per pass: what Trainer.fit takes as train_dataloaders /
    val_dataloaders for TACORL and PlayLMP (the counterpart of RelayLoader).  A training batch carries
    draw_play_batch_augmentation(aug_specs, ...); train=False (validation) draws none.  A batch is views of the replay's ring
    of buffers (HbmPlayReplay(slots=6)): a trainer may hold up to `slots - 1` batches ahead of the one it runs."""

    def __init__(self, replay, batch_size, steps_per_epoch, aug_specs=None, generator=None, train=True, fused=True):
        self.replay, self.batch_size, self.steps_per_epoch = replay, int(batch_size), int(steps_per_epoch)
        self.aug_specs, self.generator, self.train, self.fused = aug_specs, generator, train, fused

    def __len__(self):
        return self.steps_per_epoch

    def __iter__(self):
        rp = self.replay
        for _ in range(self.steps_per_epoch):
            draws = rp.index.draw_device(self.batch_size, rp.dev, self.generator)
            aug = None
            if self.train and self.aug_specs:
                aug = draw_play_batch_augmentation(self.aug_specs, self.batch_size, rp.T, rp.dev, self.generator)
            yield rp.batch(draws, aug=aug, fused=self.fused)


_INDEX_KEYS = ("min_window_size", "max_window_size", "goal_sampling_prob", "goal_strategy_prob", "goal_augmentation")
_DATASET_KEYS = _INDEX_KEYS + ("pad", "include_goal", "nn_steps_from_step", "nn_steps_from_step_val", "nn_steps_from_step_path",
                               "path", "arrays")
_DATASET_UNUSED = ("_target_", "_recursive_", "modalities", "action_type", "n_digits", "transf_type", "transform_manager",
                   "num_nn", "real_world", "skip_frames", "data_dir", "train")


class PlayDataModule:
    """Drop-in for the reference's BasicDataModule with the PlayDataset configs (config/datamodule/{tacorl,play_lmp}.yaml with
    dataset/{tacorl,play_dataset}.yaml): `Trainer.fit(model, datamodule=dm)`.  `dataset` is the reference's dataset config
    (min_window_size, max_window_size, pad, include_goal, goal_sampling_prob, goal_strategy_prob, goal_augmentation) plus
    where the data is: `path`, an .npz with `frames/<camera>` (N,H,W,3) uint8, `actions` (N,A) and the episode tables
    `ep_start_end_ids_train` / `ep_start_end_ids_val` over those N frames, or `arrays`, a dict of the same.
    include_goal false (PlayLMP's play_dataset.yaml): the batch has no `goal` and no `disp`, and no neighbour table is read.
    `nn_steps_from_step` (here or in `dataset`; `nn_steps_from_step_val` for the validation split): a NeighbourTable
    (data/neighbours.py), the reference's dict {step: [steps]}, or the path of the reference's JSON file, read with
    NeighbourTable.load_json ("train" / "validation"); the config's `nn_steps_from_step_path` is read the same way where it
    names an existing file and no table was given.  Without a table a similar_robot_obs goal is the reference's fallback, a
    random state.  train_percentage / val_percentage keep the first int(len * p) items (BasicDataModule's Subset);
    val_percentage 0: no validation loader.  pad must be true: the reference cannot collate unpadded windows of varying
    length either.  `_target_`, `modalities`, `action_type`, `n_digits`, `transf_type`, `num_nn`, `real_world`, `num_workers`,
    `pin_memory`, `shuffle_val`, `data_dir` are accepted and unused: the dataset is resident and a batch is one kernel launch.
    transform_manager: the `rl` form (see relay_replay.augment_specs); its train list becomes the train loader's
    augmentation, a Resize to the stored size is no stage, and validation batches carry no augmentation - the frames must be
    stored at the size the validation list resizes to.
    steps_per_epoch defaults to len(train index) // batch_size; batches are fresh i.i.d. device draws with replacement
    (PlayIndex.draw_device), not the reference's shuffled pass without replacement.  Validation batches are device draws
    like the training ones (as RILDataModule's): the reference chooses a validation window size with hash(str(idx)), which
    Python salts per process, so its validation set is not reproducible from run to run even there."""

    def __init__(self, dataset, batch_size=64, train_percentage=1.0, val_percentage=1.0, transform_manager=None,
                 steps_per_epoch=None, val_steps=None, num_workers=4, pin_memory=True, shuffle_val=False, data_dir=None,
                 create_vis_dataset=False, nn_steps_from_step=None, nn_steps_from_step_val=None, device=None, fused=True,
                 generator=None, slots=6, **unused):
        bad = [k for k in unused if k not in ("_target_", "_recursive_")]
        if bad:
            raise TypeError(f"PlayDataModule: unknown settings {bad}")
        if create_vis_dataset:
            raise NotImplementedError("PlayDataModule: create_vis_dataset is not built")
        self.dataset_cfg, self.batch_size = dict(dataset), int(batch_size)
        self.train_percentage, self.val_percentage = float(train_percentage), float(val_percentage)
        self.transform_manager, self.steps_per_epoch, self.val_steps = transform_manager, steps_per_epoch, val_steps
        self.device, self.fused, self.generator, self.slots = device, fused, generator, slots
        c = self.dataset_cfg
        unknown = [k for k in c if k not in _DATASET_KEYS + _DATASET_UNUSED]
        if unknown:
            raise TypeError(f"PlayDataModule: unknown dataset settings {unknown}")
        if ("path" in c) == ("arrays" in c):
            raise ValueError("PlayDataModule: give the dataset as `path` (an .npz) or as `arrays`")
        if not c.get("pad", True):
            raise NotImplementedError("PlayDataModule: pad=false (windows of varying length cannot be collated)")
        for p, name in ((self.train_percentage, "train_percentage"), (self.val_percentage, "val_percentage")):
            if not 0.0 <= p <= 1.0:
                raise ValueError(f"PlayDataModule: {name} {p} outside [0, 1]")
        self.include_goal = bool(c.get("include_goal", False))
        self.index_kwargs = {k: c[k] for k in _INDEX_KEYS if k in c}
        if "goal_strategy_prob" in self.index_kwargs:
            self.index_kwargs["goal_strategy_prob"] = dict(self.index_kwargs["goal_strategy_prob"])
        self._nn = {"train": nn_steps_from_step if nn_steps_from_step is not None else c.get("nn_steps_from_step"),
                    "validation": nn_steps_from_step_val if nn_steps_from_step_val is not None else c.get("nn_steps_from_step_val")}
        self.cams = self._cameras()
        self.aug_specs = augment_specs(self.transform_manager, self.cams, "train")  # (raises for what is not built)
        self._val_specs = augment_specs(self.transform_manager, self.cams, "validation")
        self.train_replay = self.val_replay = None

    def _cameras(self):
        c = self.dataset_cfg
        if "arrays" in c:
            a = c["arrays"]
            fr = a["frames"] if "frames" in a else {k.split("/", 1)[1]: None for k in a if k.startswith("frames/")}
            return sorted(fr)
        with np.load(c["path"]) as z:
            return sorted(k.split("/", 1)[1] for k in z.files if k.startswith("frames/"))

    def _arrays(self):
        c = self.dataset_cfg
        if "arrays" in c:
            a = c["arrays"]
            frames = a["frames"] if "frames" in a else {k.split("/", 1)[1]: v for k, v in a.items() if k.startswith("frames/")}
            return dict(frames), a["actions"], a["ep_start_end_ids_train"], a.get("ep_start_end_ids_val")
        with np.load(c["path"]) as z:
            missing = [k for k in ("actions", "ep_start_end_ids_train") if k not in z.files]
            if missing or not self.cams:
                raise KeyError(f"{c['path']}: no array named {missing or 'frames/<camera>'}")
            return ({cam: z["frames/" + cam] for cam in self.cams}, z["actions"], z["ep_start_end_ids_train"],
                    z["ep_start_end_ids_val"] if "ep_start_end_ids_val" in z.files else None)

    def _neighbours(self, split, n_frames, dev):
        """The split's nn_steps_from_step as PlayIndex takes it (a NeighbourTable or a dict), or None."""
        if not self.include_goal:
            return None
        from .neighbours import NeighbourTable

        nn = self._nn[split]
        if nn is None:
            path = self.dataset_cfg.get("nn_steps_from_step_path")
            nn = path if path and os.path.isfile(os.path.expanduser(str(path))) else None
            if nn is None and split == "validation" and isinstance(self._nn["train"], (str, os.PathLike)):
                nn = self._nn["train"]  # the reference's file holds both splits
        if isinstance(nn, (str, os.PathLike)):
            try:
                return NeighbourTable.load_json(nn, split, n_frames, device=dev)
            except KeyError:
                if split == "train":
                    raise
                return None
        return nn.to(dev) if _is_table(nn) else nn

    def _index(self, ep, percentage, split, n_frames, dev):
        ix = PlayIndex(ep, nn_steps_from_step=self._neighbours(split, n_frames, dev), train=split == "train", **self.index_kwargs)
        ix.episode_lookup = ix.episode_lookup[: int(len(ix.episode_lookup) * percentage)]  # BasicDataModule's Subset
        if len(ix) == 0:
            raise ValueError(f"PlayDataModule: the {split} index has no item (percentage {percentage})")
        return ix

    def prepare_data(self, *args, **kwargs):
        pass

    def setup(self, stage=None):
        if self.train_replay is not None:
            return
        from ..lightning import default_device

        dev = torch.device(self.device if self.device is not None else default_device())  # one process per GPU
        frames, actions, ep_train, ep_val = self._arrays()
        frames = {c: torch.as_tensor(v).to(dev).contiguous() for c, v in frames.items()}  # both splits share the frames
        acts = torch.as_tensor(np.asarray(actions, dtype=np.float32)).to(dev)
        n = min([int(v.shape[0]) for v in frames.values()] + [int(acts.shape[0])])
        for c, v in frames.items():
            stored = tuple(v.shape[1:3])
            sp, vs = self.aug_specs[c], self._val_specs[c]
            if sp is not None and sp.resize == stored:
                sp.resize = None
            resized = [s.resize for s in (sp, vs) if s is not None and s.resize not in (None, stored)]
            if resized and self.val_percentage > 0:
                raise NotImplementedError(f"{c}: validation batches carry no resize - store the frames at {resized[0]}, not {stored}")
        specs = {c: s for c, s in self.aug_specs.items() if s is not None and (s.resize is not None or s.pad or s.prob)}
        self._train_specs = specs or None
        kw = dict(device=dev, batch_size=self.batch_size, slots=self.slots, include_goal=self.include_goal)
        ix = self._index(ep_train, self.train_percentage, "train", n, dev)
        self.train_replay = HbmPlayReplay(frames, acts, ix, **kw)
        self.index = ix
        if self.val_percentage > 0:
            if ep_val is None:
                raise KeyError("PlayDataModule: val_percentage > 0 needs `ep_start_end_ids_val`")
            vix = self._index(ep_val, self.val_percentage, "validation", n, dev)
            self.val_replay = HbmPlayReplay(frames, acts, vix, **kw)
            if self.val_steps is None:
                self.val_steps = max(len(vix) // self.batch_size, 1)
        if self.steps_per_epoch is None:
            self.steps_per_epoch = len(ix) // self.batch_size
        if int(self.steps_per_epoch) < 1:
            raise ValueError(f"{len(ix)} items give no batch of {self.batch_size}")

    def train_dataloader(self):
        self.setup()
        return PlayWindowLoader(self.train_replay, self.batch_size, self.steps_per_epoch, aug_specs=self._train_specs,
                                generator=self.generator, fused=self.fused)

    def val_dataloader(self):
        self.setup()
        if self.val_replay is None:
            return None
        return PlayWindowLoader(self.val_replay, self.batch_size, self.val_steps, generator=self.generator, train=False,
                                fused=self.fused)
